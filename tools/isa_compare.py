#!/usr/bin/env python3
"""Are the existing kernels' gfx950 bodies the same in two builds of librt_hip.so?  (CPU only.)

For each library: the .hip_fatbin section's offload bundles -> their gfx950 code objects ->
`llvm-objdump -d`; then every function whose name matches `--pattern` (default: the render,
pixels, radiance, trace and occluded kernels) in the first library is compared, instruction by
instruction, with the function of the same mangled name in the second.  Prints the counts, the
names that differ or are missing, and the symbols only the second library has; exit status 1 if
any compared function differs or is missing.

python tools/isa_compare.py OLD/librt_hip.so raytracingproject_amd/lib/librt_hip.so
"""
import argparse
import re
import struct
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def functions(lib: str, arch: str) -> dict:
    """{mangled name: [instruction text, ...]} over every code object for `arch` in lib."""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        fat = Path(d) / "fatbin"
        subprocess.run([str(LLVM / "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", lib, str(fat)],
                       check=True)
        data = fat.read_bytes()
        pos, n = data.find(MAGIC), 0
        while pos >= 0:
            (count,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
            p = pos + len(MAGIC) + 8
            for _ in range(count):
                off, size, tl = struct.unpack_from("<QQQ", data, p)
                triple = data[p + 24:p + 24 + tl].decode()
                p += 24 + tl
                if arch not in triple or not size:
                    continue
                co = Path(d) / f"co{n}.co"
                n += 1
                co.write_bytes(data[pos + off:pos + off + size])
                dis = subprocess.run([str(LLVM / "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr",
                                      str(co)], capture_output=True, text=True, check=True).stdout
                cur = None
                for line in dis.splitlines():
                    m = re.match(r"^(?:[0-9a-f]+ )?<(\S+)>:$", line.strip())
                    if m:
                        cur = out.setdefault(m.group(1), [])
                    elif cur is not None and line.strip():
                        cur.append(re.sub(r"\s*//.*$", "", line).strip())
            pos = data.find(MAGIC, pos + len(MAGIC))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--pattern", default=r"render_kernel|pixels_kernel|radiance_kernel|trace_kernel|occluded_kernel")
    a = ap.parse_args()
    old, new = functions(a.old, a.arch), functions(a.new, a.arch)
    names = sorted(k for k in old if re.search(a.pattern, k))
    same = 0
    bad = []
    for k in names:
        if k not in new:
            bad.append(("missing", k))
        elif old[k] != new[k]:
            bad.append((f"differs ({len(old[k])} -> {len(new[k])} instructions)", k))
        else:
            same += 1
    for what, k in bad:
        print(what, k)
    print(f"{len(names)} functions match /{a.pattern}/: {same} identical ({sum(len(old[k]) for k in names)} "
          f"instructions), {len(bad)} different or missing")
    print("only in the new library:", *sorted(set(new) - set(old)), sep="\n  ")
    sys.exit(1 if bad or not names else 0)


if __name__ == "__main__":
    main()
