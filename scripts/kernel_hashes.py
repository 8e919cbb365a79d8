"""SHA-256 of every kernel's machine code in a gfx950 code object: the bytes [value, value + size) of each FUNC symbol.

    llvm-objdump --offloading obj/<stem>.o          # -> obj/<stem>.o.0.hipv4-amdgcn-amd-amdhsa--gfx950
    python scripts/kernel_hashes.py obj/<stem>.o.0.hipv4-amdgcn-amd-amdhsa--gfx950 | sort -u -k3

A file that gained a kernel has another code object; this shows, symbol by symbol, that the kernels it had are the same bytes
(branches are relative, so a kernel's bytes do not depend on where it lies)."""
import hashlib, os, re, subprocess, sys
path = sys.argv[1]
run = lambda *a: subprocess.run([os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "llvm-readelf"), *a, path], capture_output=True, text=True, check=True).stdout
secs = {}
for m in re.finditer(r"\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", run("-S", "-W")):
    secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))
data = open(path, "rb").read()
for line in sorted(run("-s", "-W").splitlines()):
    f = line.split()
    if len(f) == 8 and f[3] == "FUNC" and f[6].isdigit():
        val, size, (addr, off) = int(f[1], 16), int(f[2]), secs[int(f[6])]
        print(hashlib.sha256(data[off + val - addr: off + val - addr + size]).hexdigest(), size, f[7])
