#!/usr/bin/env python3
"""Basic blocks of one kernel in an assembly file that hold a given instruction, with their
instruction mix (VALU / 32-bit integer multiplies / fp64 / SALU / LDS / scalar loads / readlane).

Used to count straight-line paths that tools/isa_loops.py does not look for (it finds the
traversal loops), such as render_coherent's pop: the only code of the fp32 sphere-grid kernels
with an fp64 FMA (the tile-row decode) and a run of v_mul_lo_u32 (the three hash32 of rng.start).

python tools/isa_blocks.py FILE.s KERNEL_SUBSTRING [--has REGEX] [--min-moves N]     (--has . : every block)
(--min-moves N: only blocks with at least N v_mov_b32 / v_mov_b64, the runs of register copies;
 each such block is printed with its loop depth, and one closing line gives the share of v_mov
 among the VALU of all blocks at depth >= 2 -- depth 1 is the kernel's straight-line code and
 every enclosing natural loop adds one, so depth >= 2 is the round loop and all it holds)
(FILE.s: hipcc -S --cuda-device-only with build.py's flags; a line reads
 "block INDEX LABEL-or-%bb-number: counts")
"""
import argparse
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("kernel")
    ap.add_argument("--has", default=r"v_fma_f64|v_mul_lo_u32")
    ap.add_argument("--min-moves", type=int, default=0)
    a = ap.parse_args()
    lines = open(a.asm).read().splitlines()
    start = next(i for i, l in enumerate(lines) if re.match(r"^_Z\w+:", l) and a.kernel in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    blocks, cur = [], {"name": "entry", "ins": []}
    blocks.append(cur)
    for l in lines[start + 1:end]:
        m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %bb\.(\d+):", l)
        if m:
            cur = {"name": m.group(1), "ins": []}
            blocks.append(cur)
            continue
        t = l.split(";")[0].strip()
        if t and not t.startswith(".") and not t.endswith(":"):
            cur["ins"].append(t)

    def depths():
        """1 + the number of natural loops (merged per header) around each block."""
        idx = {b["name"]: i for i, b in enumerate(blocks)}
        n = len(blocks)
        succ = [set() for _ in range(n)]
        for i, b in enumerate(blocks):
            for t in b["ins"]:
                m = re.match(r"s_(?:cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", t)
                if m and m.group(1) in idx:
                    succ[i].add(idx[m.group(1)])
            last = b["ins"][-1] if b["ins"] else ""
            if not last.startswith(("s_branch", "s_endpgm")) and i + 1 < n:
                succ[i].add(i + 1)
        pred = [set() for _ in range(n)]
        for i, ss in enumerate(succ):
            for j in ss:
                pred[j].add(i)
        dom = [set(range(n)) for _ in range(n)]
        dom[0] = {0}
        changed = True
        while changed:
            changed = False
            for i in range(1, n):
                d = (set.intersection(*(dom[q] for q in pred[i])) if pred[i] else set()) | {i}
                if d != dom[i]:
                    dom[i], changed = d, True
        loops = {}
        for x in range(n):
            for q in pred[x]:
                if x in dom[q]:   # back edge q -> x
                    body, work = loops.setdefault(x, {x}), [q]
                    while work:
                        w = work.pop()
                        if w not in body:
                            body.add(w)
                            work.extend(pred[w])
        return [1 + sum(i in body for body in loops.values()) for i in range(n)]

    def mix(ins):
        c = dict(valu=0, imul=0, f64=0, salu=0, lds=0, smem=0, readlane=0, vmem=0, branch=0, mov=0)
        for t in ins:
            op = t.split()[0]
            if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane")):
                c["readlane"] += 1
                c["valu"] += 1
            elif op.startswith("v_"):
                c["valu"] += 1
                c["imul"] += op.startswith(("v_mul_lo_u32", "v_mul_hi_u32", "v_mad_u64_u32", "v_mul_lo_i32"))
                c["f64"] += "f64" in op
                c["mov"] += op.startswith(("v_mov_b32", "v_mov_b64"))
            elif op.startswith(("s_load", "s_buffer_load")):
                c["smem"] += 1
            elif op.startswith(("s_cbranch", "s_branch")):
                c["branch"] += 1
            elif op.startswith("s_"):
                c["salu"] += 1
            elif op.startswith("ds_"):
                c["lds"] += 1
            elif op.startswith(("global_", "scratch_", "flat_", "buffer_")):
                c["vmem"] += 1
        return c

    tot = None
    depth = depths() if a.min_moves else None
    for k, b in enumerate(blocks):
        if not any(re.search(a.has, t) for t in b["ins"]):
            continue
        c = mix(b["ins"])
        if c["mov"] < a.min_moves:
            continue
        print(f"block {k} {b['name']}: " + " ".join(f"{n}={v}" for n, v in c.items()) +
              (f" depth={depth[k]}" if depth else ""))
        tot = c if tot is None else {n: tot[n] + c[n] for n in c}
    if tot:
        print("sum: " + " ".join(f"{n}={v}" for n, v in tot.items()))
    if depth:
        inner = [mix(b["ins"]) for k, b in enumerate(blocks) if depth[k] >= 2]
        valu, mov = sum(c["valu"] for c in inner), sum(c["mov"] for c in inner)
        print(f"depth >= 2: {len(inner)} blocks, v_mov {mov} of {valu} VALU ({mov / max(1, valu):.1%})")


if __name__ == "__main__":
    main()
