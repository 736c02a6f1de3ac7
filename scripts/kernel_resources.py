"""Per-kernel VGPRs / spills / LDS / occupancy of a HIP source (hipcc
-Rpass-analysis=kernel-resource-usage): python scripts/kernel_resources.py <src.hip> [name-substring]
[extra hipcc flags...].  Compiles to /tmp with the flags the production build uses for that file
(analyzer_amd/build_ext.py HIP_FLAGS); prints one line per kernel."""
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from analyzer_amd import build_ext  # noqa: E402

src = sys.argv[1]
sub = sys.argv[2] if len(sys.argv) > 2 else ""
extra = sys.argv[3:]
cmd = ["hipcc", "--offload-arch=" + build_ext.ARCH, "-O3", "-std=c++17", "-fPIC", "-I" + str(build_ext.CSRC)]
cmd += build_ext.HIP_FLAGS.get(os.path.basename(src), [])
cmd += ["-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", "/tmp/kernel_resources.o"] + extra
out = subprocess.run(cmd, capture_output=True, text=True).stderr
cur, rows = None, []
for line in out.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = {"name": m.group(1)}
        rows.append(cur)
        continue
    m = re.search(r"remark: ([A-Za-z /\[\]]+?): (\S+) \[-Rpass", line)
    if m and cur is not None:
        cur[m.group(1).strip()] = m.group(2)
for r in rows:
    if sub in r["name"]:
        print("%-70s VGPRs %4s  AGPRs %3s  VGPR spill %3s  SGPR spill %3s  LDS %6s  occupancy %s" % (
            r["name"][:70], r.get("VGPRs"), r.get("AGPRs"), r.get("VGPRs Spill"), r.get("SGPRs Spill"),
            r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]")))
