#!/usr/bin/env python3
"""Are the existing kernels' gfx950 bodies the same in two builds of librt_hip.so?  (CPU only.)

For each library: the .hip_fatbin section's offload bundles -> their gfx950 code objects ->
`llvm-objdump -d`; then every function whose name matches `--pattern` (default: the render,
pixels, moments, aov, radiance, trace and occluded kernels) in the first library is compared,
instruction by instruction, with the function of the same mangled name in the second.  Prints the
counts, the names that differ or are missing -- for one that differs also its registers, spills,
scratch and LDS in both libraries (`llvm-readelf --notes`), the figures that changed marked --
and the symbols only the second library has; exit status 1 if any compared function differs or
is missing.

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


NOTES = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size", "sgpr_count",
         "sgpr_spill_count")


def functions(lib: str, arch: str) -> tuple:
    """{mangled name: [instruction text, ...]} and {kernel name: {NOTES field: value}} over every
    code object for `arch` in lib."""
    out, meta = {}, {}
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
                # the metadata lists a kernel's fields in alphabetical order: .name after .agpr_count
                # and .group_segment_fixed_size, before the rest
                notes = subprocess.run([str(LLVM / "llvm-readelf"), "--notes", str(co)], capture_output=True,
                                       text=True, check=True).stdout
                for kern in notes.split("- .agpr_count:")[1:]:
                    f = dict(re.findall(r"^\s+\.(\w+):\s+(\S+)\s*$", kern, re.M))
                    meta[f["name"]] = {k: int(f[k]) for k in NOTES}
            pos = data.find(MAGIC, pos + len(MAGIC))
    return out, meta


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--pattern", default=r"render_kernel|pixels_kernel|pixels_moments_kernel|aov_kernel|radiance_kernel|"
                                         r"trace_kernel|occluded_kernel")
    a = ap.parse_args()
    (old, old_meta), (new, new_meta) = functions(a.old, a.arch), functions(a.new, a.arch)
    names = sorted(k for k in old if re.search(a.pattern, k))
    same = 0
    bad = []
    for k in names:
        if k not in new:
            bad.append(("missing", k))
        elif old[k] != new[k]:
            m = "".join(f" {f} {old_meta[k][f]} -> {new_meta[k][f]}{'' if old_meta[k][f] == new_meta[k][f] else ' (!)'},"
                        for f in NOTES) if k in old_meta and k in new_meta else ""
            bad.append((f"differs ({len(old[k])} -> {len(new[k])} instructions;{m.rstrip(',')})", k))
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
