#!/usr/bin/env python3
"""Instruction counts of a kernel's largest loop body in hipcc -S output (the step kernels' substep loop).

The body is the code between the target of the kernel's longest backward branch and that branch.
Prints one JSON line per kernel matched: whole-kernel and body totals, and the body split into VALU, DS
(LDS), SALU, s_waitcnt, s_nop, v_add_u32, v_readlane/v_writelane, the wide LDS forms (b64/b96/b128) and
the two-address forms (read2/write2), plus the kernel's resource directives.

usage: python tools/isa_loop_count.py [--scene flat] [--kernel step_kernelI] [--asm FILE] [-D DEFINE ...]
Without --asm the scene's unit is compiled with native.compile_flags() into a temporary file."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

WIDE = re.compile(r"^ds_(read|write)_b(64|96|128)\b")
TWO = re.compile(r"^ds_(read|write)2(st64)?_b(32|64)\b")
RES = (".vgpr_count", ".agpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def functions(text):
    """name -> list of (labels seen so far, mnemonic, operands) per instruction"""
    out, cur, name = {}, None, None
    for line in text.splitlines():
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^([A-Za-z_.$][\w.$]*):$", s)
        if m:
            lab = m.group(1)
            if not lab.startswith(".L"):
                name, cur = lab, []
                out[name] = cur
            elif cur is not None:
                cur.append(("label", lab, ""))
            continue
        if s.startswith(".") or cur is None:
            if s.startswith(".end_amdhsa_kernel") or s.startswith(".Lfunc_end"):
                cur = None
            continue
        parts = s.split(None, 1)
        cur.append(("ins", parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def classify(ins):
    c = dict(total=len(ins), valu=0, ds=0, salu=0, waitcnt=0, nop=0, v_add_u32=0, lane_rw=0, ds_wide=0, ds_two=0,
             vmem=0)
    for op, _ in ins:
        if op.startswith("s_waitcnt"):
            c["waitcnt"] += 1
        elif op == "s_nop":
            c["nop"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["ds"] += 1
            c["ds_wide"] += bool(WIDE.match(op))
            c["ds_two"] += bool(TWO.match(op))
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
            c["v_add_u32"] += op.startswith("v_add_u32")
            c["lane_rw"] += op.startswith(("v_readlane", "v_writelane"))
    return c


def loop_body(items):
    pos, k = {}, 0
    ins = []
    for kind, a, b in items:
        if kind == "label":
            pos[a] = k
        else:
            ins.append((a, b))
            k += 1
    best = (0, 0, 0)
    for i, (op, args) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")):
            t = pos.get(args.strip())
            if t is not None and t <= i and i - t > best[0]:
                best = (i - t, t, i)
    return ins, ins[best[1]:best[2] + 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="flat")
    ap.add_argument("--kernel", default="step_kernelI", help="substring of the mangled kernel name")
    ap.add_argument("--asm")
    ap.add_argument("-D", action="append", default=[])
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        from open_duck_playground_amd import native
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "unit.s")
            subprocess.check_call(["hipcc"] + native.compile_flags() + [f"-D{d}" for d in a.D] +
                                  ["--cuda-device-only", "-S", "-o", out,
                                   os.path.join(native.CSRC, f"variant_{a.scene}.hip")], cwd=native.CSRC)
            text = open(out).read()
    res = {}
    # resource entries of the metadata block: "- .agpr_count: N ... .name: K ... .vgpr_count: N"
    for blk in re.split(r"\n\s+- \.agpr_count:", text)[1:]:
        blk = ".agpr_count:" + blk
        nm = re.search(r"\.name:\s+(\S+)", blk)
        if nm:
            res[nm.group(1)] = {k[1:]: int(v) for k in RES for v in re.findall(re.escape(k) + r":\s+(\d+)", blk)[:1]}
    for name, items in functions(text).items():
        if a.kernel not in name or not name.startswith("_Z"):
            continue
        ins, body = loop_body(items)
        print(json.dumps({"kernel": name[:60], "whole": classify(ins), "body": classify(body),
                          "resources": res.get(name, {})}))


if __name__ == "__main__":
    main()
