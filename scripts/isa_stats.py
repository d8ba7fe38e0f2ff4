#!/usr/bin/env python3
"""Static picture of the gfx950 code of selected kernels: instruction mix, registers, scratch, LDS.

    python scripts/isa_stats.py k_ndt_pass k_gicp_linearize            # compiles hgs_kernels.hip with --save-temps into /tmp/hgs_isa
    python scripts/isa_stats.py --asm /tmp/hgs_isa/x.s k_knn_cov
    python scripts/isa_stats.py --blocks "k_fitness<hgs::TargetView>"            # instruction mix per basic block of the kernel's loops

Counts are of the kernel's TEXT (every instruction once, whatever the loop structure): what a change did to the register budget, the
scratch frame and the kind of instructions issued — not how often they run (that is rocprofv3 --pmc's SQ_INSTS_*).
"""
from __future__ import annotations

import argparse
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def compile_asm(extra):
    out = "/tmp/hgs_isa"
    os.makedirs(out, exist_ok=True)
    cmd = ["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-function", "--save-temps", *extra, "-c",
           os.path.join(ROOT, "hdl_graph_slam_amd", "csrc", "hgs_kernels.hip"), "-o", "k.o"]
    subprocess.run(cmd, cwd=out, check=True, stderr=subprocess.DEVNULL)
    return os.path.join(out, "hgs_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")


def kernels(asm):
    text = open(asm).read()
    for m in re.finditer(r"\n(_Z\w+):[^\n]*\n(.*?)\n\t\.amdhsa_kernel \1\n(.*?)\.end_amdhsa_kernel", text, re.S):
        yield m.group(1), m.group(2), m.group(3)


def demangle(name):
    try:
        return subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-cxxfilt", name], capture_output=True, text=True).stdout.strip().split("(")[0]
    except OSError:
        return name


def classify(op):
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "other"


def loop_blocks(body):
    """The basic blocks of a kernel's loops, in text order: (label, loop, depth, is_header, [opcodes]).  A block starts at a label or at a
    `; %bb.N:` line; the compiler's comments say which loop it belongs to (`in Loop: Header=BBx_y Depth=d`, `Loop Header: Depth=d`)."""
    blocks, cur = [], None
    for line in body.split("\n"):
        m = re.match(r"(\.LBB\d+_\d+):|; %bb\.(\d+):", line)
        if m:
            cur = {"label": m.group(1) or "bb." + m.group(2), "loop": None, "depth": 0, "header": False, "ops": []}
            blocks.append(cur)
        if cur is None:
            continue
        m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", line)
        if m and not cur["header"]:
            cur["loop"], cur["depth"] = m.group(1), int(m.group(2))
        m = re.search(r"Loop Header: Depth[= ](\d+)", line)
        if m:
            cur["loop"], cur["depth"], cur["header"] = cur["label"].lstrip(".L"), int(m.group(1)), True
        if line.startswith("\t") and not line.lstrip().startswith((".", ";")):
            cur["ops"].append(line.split()[0])
    return [b for b in blocks if b["loop"]]


def print_blocks(pretty, body, detail):
    """Instruction mix per basic block of the kernel's loops (text counts: one pass through the block)."""
    print(pretty)
    print("   block        loop         depth  instr  salu  valu  lds  vmem   (of salu: waitcnt / branch)")
    for b in loop_blocks(body):
        c = collections.Counter(classify(op) for op in b["ops"])
        wait = sum(op in ("s_waitcnt", "s_nop") for op in b["ops"])
        br = sum(op.startswith(("s_cbranch", "s_branch")) for op in b["ops"])
        head = "*" if b["header"] else " "
        print(f"  {head}{b['label']:<12} {b['loop']:<12} {b['depth']:>5}  {len(b['ops']):>5} {c['salu']:>5} {c['valu']:>5} {c['lds']:>4} {c['vmem']:>5}   ({wait} / {br})")
        if detail:
            for op, n in sorted(collections.Counter(b["ops"]).items()):
                print(f"        {n:>3} {op}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("patterns", nargs="+")
    ap.add_argument("--asm")
    ap.add_argument("-D", action="append", default=[])
    ap.add_argument("--blocks", action="store_true", help="instruction mix per basic block of the kernel's loops (* marks a loop header)")
    ap.add_argument("--detail", action="store_true", help="with --blocks: the opcodes of every block")
    a = ap.parse_args()
    asm = a.asm or compile_asm(["-D" + d for d in a.D])
    for name, body, meta in kernels(asm):
        pretty = demangle(name)
        if not any(p in pretty or p in name for p in a.patterns):   # (the mangled name serves where no demangler is installed)
            continue
        if a.blocks:
            print_blocks(pretty, body, a.detail)
            continue
        ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.lstrip().startswith((".", ";"))]
        c = collections.Counter(ins)
        grp = collections.Counter()
        for k, v in c.items():
            if k.startswith("v_mfma"):
                grp["mfma"] += v
            elif k.startswith("v_pk_"):
                grp["valu_pk"] += v
            elif k.startswith("v_") and "f64" in k:
                grp["valu_f64"] += v
            elif k.startswith("v_"):
                grp["valu_other"] += v
            elif k.startswith("s_"):
                grp["salu"] += v
            elif k.startswith("ds_"):
                grp["lds"] += v
            elif k.startswith(("global_", "flat_", "buffer_")):
                grp["vmem"] += v
            elif k.startswith("scratch_"):
                grp["scratch"] += v
        def field(key):
            m = re.search(r"\." + key + r"\s+(\d+)", meta)
            return int(m.group(1)) if m else None
        print(f"{pretty}")
        print(f"   instructions {len(ins)}: " + ", ".join(f"{k} {v}" for k, v in sorted(grp.items())))
        print(f"   next_free_vgpr {field('amdhsa_next_free_vgpr')}  accum_offset {field('amdhsa_accum_offset')}  next_free_sgpr {field('amdhsa_next_free_sgpr')}  "
              f"scratch {field('amdhsa_private_segment_fixed_size')} B  LDS {field('amdhsa_group_segment_fixed_size')} B")
        top = ", ".join(f"{k} {v}" for k, v in c.most_common(12))
        print(f"   top: {top}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
