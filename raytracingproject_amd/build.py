"""Build the native library in-tree: raytracingproject_amd/lib/librt_hip.so.

hipcc cross-compiles for gfx950 (MI355X) without a GPU present.  The two kernel
translation units differ only in FP contraction: the fp32 fast path may fuse into FMAs,
the fp64 reference-exact path may not (-ffp-contract=off) so that its roundings are
those of the g++-built reference.
"""
from __future__ import annotations

import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
OBJ = PKG / "build"
LIB = PKG / "lib" / "librt_hip.so"
ARCH = os.environ.get("RT_OFFLOAD_ARCH", "gfx950")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

COMMON = ["-x", "hip", f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-Wall",
          "-Wno-unused-function", f"-I{ROOT / 'include'}"] + os.environ.get("RT_HIPCC_EXTRA", "").split()
F32_FAST = ["-fno-hip-fp32-correctly-rounded-divide-sqrt", "-fgpu-flush-denormals-to-zero",
            os.environ.get("RT_F32_CONTRACT", "-ffp-contract=on")]
UNITS = {
    "rt_render_f32.hip": F32_FAST,
    # the fp32 job-list query kernels over the sphere grid: rt_render_f32.hip's flags, so its arithmetic
    "rt_query_grid_f32.hip": F32_FAST,
    "rt_render_f64.hip": ["-ffp-contract=off"],
    "rt_abi.cpp": ["-ffp-contract=off"],
    "rt_plan.cpp": ["-ffp-contract=off"],
    "rt_pack.cpp": ["-ffp-contract=off"],
    "rt_bvh.cpp": ["-ffp-contract=off"],
    "rt_obj.cpp": ["-ffp-contract=off"],
    "rt_lbvh.hip": ["-ffp-contract=off"],
    # rt_denoise's rule is bit-exact in fp32 too: no contraction, IEEE divide / sqrt, denormals kept
    "rt_denoise.hip": ["-ffp-contract=off"],
    "rt_comm.cpp": [],
}
HEADERS = ["rt_device.h", "rt_render_impl.h", "rt_occluded.h", "rt_radiance.h", "rt_pixels.h", "rt_moments.h", "rt_aov.h", "rt_scene.h", "rt_launch.h", "rt_bvh.h", "rt_lbvh.h", "rt_ctx.h", "rt_devbuf.h",
           "rt_treelet.h", "rt_pack.h", "rt_batch_cull.h", "rt_denoise.h", "rt_quant.h", "rt_trav.h"]


def _stale(target: Path, deps: list[Path]) -> bool:
    if not target.exists():
        return True
    t = target.stat().st_mtime
    return any(d.stat().st_mtime > t for d in deps)


def _present(p: Path) -> bool:
    """p.exists(), where a path this user may not look at counts as absent."""
    try:
        return p.exists()
    except OSError:
        return False


def _compile(src: str, extra: list[str], verbose: bool) -> Path:
    obj = OBJ / (src.rsplit(".", 1)[0] + ".o")
    # build.py itself: a changed flag rebuilds every object
    deps = [CSRC / src] + [CSRC / h for h in HEADERS] + [ROOT / "include" / "rt_hip.h", Path(__file__)]
    if _stale(obj, deps):
        cmd = [HIPCC, *COMMON, *extra, "-c", str(CSRC / src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return obj


def build_native(verbose: bool = False) -> Path:
    OBJ.mkdir(parents=True, exist_ok=True)
    LIB.parent.mkdir(parents=True, exist_ok=True)
    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(lambda kv: _compile(kv[0], kv[1], verbose), UNITS.items()))
    if _stale(LIB, objs):
        cmd = [HIPCC, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", str(LIB), *map(str, objs),
               "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return LIB


def build_dropin(verbose: bool = False) -> list[Path]:
    """C++ programs over the drop-in headers (include/rt) linked to librt_hip.so:
    examples/pixelmatch.cpp always; and, where /root/reference exists, the reference's
    own src/main.cpp compiled UNCHANGED against include/rt (fed on stdin from the
    include/rt directory so that its quoted includes resolve to the drop-in headers;
    nothing is copied)."""
    out_dir = ROOT / "examples" / "_build"
    out_dir.mkdir(parents=True, exist_ok=True)
    inc = ROOT / "include" / "rt"
    link = [f"-L{LIB.parent}", "-lrt_hip", f"-Wl,-rpath,{LIB.parent}", "-Wl,-rpath,$ORIGIN/../../raytracingproject_amd/lib"]
    built = []
    for name in ("pixelmatch", "host_queries", "mesh_scene"):
        exe = out_dir / name
        src = ROOT / "examples" / f"{name}.cpp"
        if _stale(exe, [src, LIB, *inc.glob("*.h")]):
            subprocess.run(["g++", "-O2", "-std=c++17", f"-I{inc}", str(src), "-o", str(exe), *link], check=True)
        built.append(exe)
    ref_main = Path("/root/reference/src/main.cpp")
    if _present(ref_main):
        exe = out_dir / "reference_main_on_mi355x"
        if _stale(exe, [ref_main, LIB, *inc.glob("*.h")]):
            with open(ref_main, "rb") as f:
                subprocess.run(["g++", "-O2", "-std=c++17", "-x", "c++", "-", f"-I{inc}", "-o", str(exe), *link],
                               check=True, stdin=f, cwd=inc)
        built.append(exe)
    return built


SAN_FLAGS = ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all"]
SAN_EXE = OBJ / "san" / "san_driver"
INC = f"-I{ROOT / 'include'}"


def _build_san(exe: Path, srcs: list[Path], deps: list[Path], extra=(), verbose: bool = False) -> Path:
    """One stand-alone g++ program under SAN_FLAGS: srcs (sources, or objects built before) with
    `extra` flags into exe, when it is older than srcs, deps or this file.  No GPU code."""
    exe.parent.mkdir(parents=True, exist_ok=True)
    if _stale(exe, [*srcs, *deps, Path(__file__)]):
        cmd = ["g++", "-std=c++17", *SAN_FLAGS, *extra, *map(str, srcs), "-o", str(exe), "-lm"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return exe


def build_sanitize(verbose: bool = False) -> Path:
    """Host-only sanitizer build (the reference's ASan flags are commented
    out, CMakeLists.txt:18-23): the product's host sources that take untrusted input or
    build the trees (csrc/rt_obj.cpp, csrc/rt_bvh.cpp) and the oracle (oracle/rt_oracle.c)
    compiled with g++/gcc -fsanitize=address,undefined into one driver,
    tests/cpp/sanitize_driver.cpp (run by tests/test_sanitize.py).  No GPU code."""
    SAN_EXE.parent.mkdir(parents=True, exist_ok=True)
    orc, oo = ROOT / "oracle" / "rt_oracle.c", SAN_EXE.parent / "rt_oracle.o"
    if _stale(oo, [orc, ROOT / "oracle" / "rt_oracle.h", Path(__file__)]):
        cmd = ["gcc", "-std=c11", *SAN_FLAGS, "-c", str(orc), "-o", str(oo)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    srcs = [ROOT / "tests" / "cpp" / "sanitize_driver.cpp", CSRC / "rt_obj.cpp", CSRC / "rt_bvh.cpp", oo]
    deps = [CSRC / "rt_bvh.h", CSRC / "rt_scene.h", ROOT / "include" / "rt_hip.h", ROOT / "oracle" / "rt_oracle.h"]
    return _build_san(SAN_EXE, srcs, deps, [INC], verbose)


RESUME_EXE = OBJ / "san" / "grid_resume_driver"
BOXES_EXE = OBJ / "san" / "bvh_boxes_driver"
PACK_EXE = OBJ / "san" / "pack_driver"
DEVBUF_EXE = OBJ / "san" / "devbuf_driver"
BVH_DEPS = [CSRC / "rt_bvh.h", CSRC / "rt_scene.h", ROOT / "include" / "rt_hip.h"]


def build_grid_resume(verbose: bool = False) -> Path:
    """tests/cpp/grid_resume_driver.cpp (the flat grid walk with suspension, restated for the
    CPU; run by tests/test_grid_resume.py) with csrc/rt_bvh.cpp, which builds its grids, under
    the same sanitizers as build_sanitize.  No GPU code."""
    srcs = [ROOT / "tests" / "cpp" / "grid_resume_driver.cpp", CSRC / "rt_bvh.cpp"]
    return _build_san(RESUME_EXE, srcs, BVH_DEPS, ["-ffp-contract=off", INC], verbose)


def build_bvh_boxes(verbose: bool = False) -> Path:
    """tests/cpp/bvh_boxes_driver.cpp (the sphere tree's boxes and the sphere grid over scenes
    with negative radii; run by tests/test_bvh_boxes.py) with csrc/rt_bvh.cpp, which builds
    both, under the same sanitizers as build_sanitize.  No GPU code."""
    srcs = [ROOT / "tests" / "cpp" / "bvh_boxes_driver.cpp", CSRC / "rt_bvh.cpp"]
    return _build_san(BOXES_EXE, srcs, BVH_DEPS, ["-ffp-contract=off", INC], verbose)


def build_pack(verbose: bool = False) -> Path:
    """tests/cpp/pack_driver.cpp (the host-side scene packing and the sphere grid's reach test;
    run by tests/test_pack.py) with csrc/rt_pack.cpp and csrc/rt_bvh.cpp, under the same
    sanitizers as build_sanitize.  No GPU code."""
    srcs = [ROOT / "tests" / "cpp" / "pack_driver.cpp", CSRC / "rt_pack.cpp", CSRC / "rt_bvh.cpp"]
    return _build_san(PACK_EXE, srcs, [CSRC / "rt_pack.h", *BVH_DEPS], ["-ffp-contract=off", INC], verbose)


def build_devbuf(verbose: bool = False) -> Path:
    """tests/cpp/devbuf_driver.cpp (csrc/rt_devbuf.h over counting fakes of the HIP calls it
    makes; run by tests/test_devbuf.py), under the same sanitizers as build_sanitize.  Only
    HIP's headers are used: no HIP library is linked, and no GPU code."""
    extra = ["-D__HIP_PLATFORM_AMD__", f"-I{CSRC}", "-I/opt/rocm/include"]
    return _build_san(DEVBUF_EXE, [ROOT / "tests" / "cpp" / "devbuf_driver.cpp"], [CSRC / "rt_devbuf.h"], extra, verbose)


QUANT_EXE = OBJ / "san" / "quant_range_driver"


def build_quant_range(verbose: bool = False) -> Path:
    """tests/cpp/quant_range_driver.cpp (the finish path's range test of csrc/rt_quant.h and what a
    finished sample adds to the frame, before and after the lean finish, over every bit pattern of
    a channel; run by tests/test_quant_range.py).  Plain g++ -O2, no sanitizer: the driver owns no
    memory and runs 2^33 samples.  No GPU code."""
    src = ROOT / "tests" / "cpp" / "quant_range_driver.cpp"
    QUANT_EXE.parent.mkdir(parents=True, exist_ok=True)
    if _stale(QUANT_EXE, [src, CSRC / "rt_quant.h", CSRC / "rt_scene.h", Path(__file__)]):
        cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-pthread", f"-I{CSRC}", INC, str(src), "-o", str(QUANT_EXE)]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return QUANT_EXE


CULL_EXE = OBJ / "san" / "batch_cull_driver"
CULL_MUTANTS = (1, 2, 3)   # rt_batch_cull.h RT_CULL_MUTATE: no margins, no lens radius, no motion half-length


def build_batch_cull(verbose: bool = False) -> list[Path]:
    """tests/cpp/batch_cull_driver.cpp (the tile / sphere cull of csrc/rt_batch_cull.h against
    brute force over fp64 camera rays; run by tests/test_batch_cull.py) under the same sanitizers
    as build_sanitize: the driver itself, then one copy per mutation of the predicate, each of
    which the driver must catch.  No GPU code."""
    src = ROOT / "tests" / "cpp" / "batch_cull_driver.cpp"
    deps = [CSRC / "rt_batch_cull.h", CSRC / "rt_scene.h"]
    exes = [CULL_EXE] + [CULL_EXE.with_name(f"batch_cull_driver_m{m}") for m in CULL_MUTANTS]

    def one(k: int) -> None:
        # (-O2 after SAN_FLAGS' -O1: the brute force is a billion flops)
        _build_san(exes[k], [src], deps, ["-O2", "-ffp-contract=off", f"-DRT_CULL_MUTATE={k}", f"-I{CSRC}"], verbose)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(one, range(len(exes))))
    return exes


DEPTH_EXE = OBJ / "san" / "cand_depth_driver"
DEPTH_MUTANTS = (1, 2, 3, 4)   # RT_CULL_MUTATE: CULL_MUTANTS' three, and the packed bound rounded up


def build_cand_depth(verbose: bool = False) -> list[Path]:
    """tests/cpp/cand_depth_driver.cpp (the candidates' near bound of csrc/rt_batch_cull.h --
    cull_near, the packed list word and its order -- against the fp32 roots of brute-forced camera
    rays; run by tests/test_cand_depth.py) under the same sanitizers as build_sanitize: the driver
    itself, then one copy per mutation of the bound, each of which the driver must catch.  No GPU
    code."""
    src = ROOT / "tests" / "cpp" / "cand_depth_driver.cpp"
    deps = [CSRC / "rt_batch_cull.h", CSRC / "rt_scene.h"]
    exes = [DEPTH_EXE] + [DEPTH_EXE.with_name(f"cand_depth_driver_m{m}") for m in DEPTH_MUTANTS]

    def one(k: int) -> None:
        _build_san(exes[k], [src], deps, ["-O2", "-ffp-contract=off", f"-DRT_CULL_MUTATE={k}", f"-I{CSRC}"], verbose)

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(one, range(len(exes))))
    return exes


def build_oracle(verbose: bool = False) -> None:
    """Compile the C restatement (test infrastructure) and, where /root/reference is
    present, the reference driver into oracle/_ref (test infrastructure: oracle/_ref/
    ref_golden ships to the GPU box as bench.py's CPU-baseline binary, and the product
    never loads either)."""
    oracle = ROOT / "oracle"
    out = None if verbose else subprocess.DEVNULL
    subprocess.run(["make", "-C", str(oracle), "liboracle.so", "rt_oracle_cli", "ref-if-present"], check=True,
                   stdout=out)


if __name__ == "__main__":
    import sys
    if "--sanitize" in sys.argv[1:]:
        print(build_sanitize(verbose=True))
        sys.exit(0)
    print(build_native(verbose=True))
    print(build_dropin(verbose=True))
    build_oracle(verbose=True)
