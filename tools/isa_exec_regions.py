#!/usr/bin/env python3
"""The exec-masked regions of a kernel's largest loop body, from hipcc -S output (CPU only).

The step kernels run one wave per SIMD, so every instruction slot of the substep body counts, and a
lane-divergent `if` costs slots that compute nothing: the s_*_saveexec that opens it, the
s_cbranch_execz the compiler keeps in front of any region with an LDS operation, and the exec restore
at the join. For the body that tools/isa_loop_count.py finds (the substep loop) this lists every
region between an exec save and the restore that closes it:
  - offset in the body, size in instructions, nesting depth (0 = top level), stage (the
    "; STAGE_MARK ST_x" comments of a -DDUCK_ASM_MARKS build, as tools/isa_wait_cover.py reads them);
  - whether an s_cbranch_execz follows the save (the branch is retained);
  - the guard: "cmp" when the mask the save reads is written by a v_cmp within the GUARD_WINDOW
    instructions in front of it, "mask" when it is an SGPR pair live from outside (a hoisted lane
    predicate: lane == 0, lane < k), "mask-spill" when that pair was just reloaded by v_readlane;
  - the contents: LDS writes, LDS reads, VALU, global / scratch memory operations (nested regions
    count towards their parents).
A region is "store-only" when it holds at least one LDS write, no LDS read, no memory operation and
no more VALU instructions than LDS writes (address arithmetic). The totals count the regions, the
retained branches, every s_cbranch_execz of the body, and the v_readlane / v_writelane of the body
(the SGPR spills of the hoisted lane masks among them).

usage: python tools/isa_exec_regions.py [--scene flat] [--kernel step_kernelI] [--asm FILE] [--json]
                                        [--totals] [-D DEFINE ...]
Without --asm the scene's unit is compiled with native.compile_flags() and -DDUCK_ASM_MARKS."""
import argparse
import collections
import json
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_loop_count as ilc  # noqa: E402
import isa_wait_cover as iwc  # noqa: E402

SAVEEXEC = re.compile(r"^s_(and|andn2|or|xor|nand|nor|orn2|xnor|andn1|orn1)_saveexec_b64$")
GUARD_WINDOW = 12  # a compare this close in front of the save is the region's own data test
BRANCH_WINDOW = 3  # s_cbranch_execz within this many instructions after the save belongs to it
SMALL = 45  # the "small region" bound of the census


def ops_of(args):
    return [a.strip() for a in args.split(",")]


def writes_exec(op, args):
    return op.startswith("s_") and not op.startswith("s_cbranch") and ops_of(args)[0] == "exec"


def guard_of(ins, i, src):
    """How the mask `src` that the save at ins[i] reads was made: cmp / mask / mask-spill"""
    if src == "exec":
        return "cmp"  # v_cmpx wrote exec itself
    lo_reg = re.match(r"s\[(\d+):", src)
    for j in range(i - 1, max(i - 1 - GUARD_WINDOW, -1), -1):
        op, args = ins[j]
        if op.startswith(iwc.TERM):
            break
        dst = ops_of(args)[0] if args else ""
        if op.startswith("v_cmp") and (dst == src or (src == "vcc" and "_e32" in op)):
            return "cmp"
        if op.startswith(("s_and_b64", "s_or_b64", "s_andn2_b64", "s_xor_b64", "s_orn2_b64")) and dst == src:
            # a combination of masks: a data test if any operand is a fresh compare, else still a mask
            rest = ops_of(args)[1:]
            kinds = [guard_of(ins, j, r) for r in rest if r.startswith(("s[", "vcc"))]
            return "cmp" if "cmp" in kinds else ("mask-spill" if "mask-spill" in kinds else "mask")
        if op.startswith("v_readlane") and lo_reg and dst in (f"s{lo_reg.group(1)}", f"s{int(lo_reg.group(1)) + 1}"):
            return "mask-spill"
    return "mask"


def regions(items, whole=False):
    """items: isa_loop_count.functions()'s list of one kernel, from isa_wait_cover.annotate()d text.
    Returns (regions, totals); a region is a dict (see the module docstring)."""
    lo, hi = (0, sum(k == "ins" for k, _, _ in items) - 1) if whole else iwc.body_range(items)
    ins, stage_at, pending = [], {}, []
    for kind, a, b in items:
        if kind == "ins":
            pending.append(len(ins))
            ins.append((a, b))
        elif a.startswith(iwc.MARK):
            for p in pending:
                stage_at[p] = a[len(iwc.MARK):].rsplit(".", 1)[0]
            pending = []
    out, stack = [], []

    def open_region(i, src, saved):
        follow = [ins[j][0] for j in range(i + 1, min(i + 1 + BRANCH_WINDOW, hi + 1))]
        stack.append(dict(offset=i - lo, start=i, depth=len(stack), stage=stage_at.get(i, "(after last mark)"),
                          branch="s_cbranch_execz" in follow, guard=guard_of(ins, i, src), saved=saved))

    def close_region(i):
        r = stack.pop()
        body = ins[r["start"] + 1:i]
        r["size"] = len(body)
        r["lds_write"] = sum(op.startswith(("ds_write", "ds_store")) for op, _ in body)
        r["lds_read"] = sum(op.startswith(("ds_read", "ds_load")) for op, _ in body)
        r["valu"] = sum(op.startswith("v_") for op, _ in body)
        r["vmem"] = sum(op.startswith(("global_", "flat_", "buffer_", "scratch_")) for op, _ in body)
        r["store_only"] = r["lds_write"] > 0 and not r["lds_read"] and not r["vmem"] and r["valu"] <= r["lds_write"]
        del r["start"], r["saved"]
        out.append(r)

    def restore(i, reg):
        """exec restored from `reg`: the join of the region that saved it and of every region opened inside
        (an if / else joins straight to the outer save); an unknown register (a reloaded spill) joins the
        innermost region"""
        if not stack:
            return
        n = 1
        for d in range(len(stack) - 1, -1, -1):
            if stack[d]["saved"] == reg:
                n = len(stack) - d
                break
        for _ in range(n):
            close_region(i)

    for i in range(lo, hi + 1):
        op, args = ins[i]
        a = ops_of(args) if args else []
        if SAVEEXEC.match(op):
            # the else flip of an if / else (s_or_saveexec / s_andn2_saveexec of the `then` side's saved
            # mask): the join of the `then` side and the save of the `else` side
            if stack and len(a) > 1 and a[1] == stack[-1]["saved"]:
                close_region(i)
            open_region(i, a[1] if len(a) > 1 else "", a[0] if a else "")
        elif op.startswith("v_cmpx"):
            open_region(i, "exec", "")
        elif writes_exec(op, args):
            if op == "s_or_b64":
                restore(i, a[-1])
            elif op == "s_mov_b64":
                if any(r["saved"] == a[1] for r in stack):
                    restore(i, a[1])
                else:
                    # s_mov_b64 sY, exec ... s_mov_b64 exec, sX: a save and a narrowing written apart
                    saved = [ops_of(ins[j][1])[0] for j in range(max(lo, i - GUARD_WINDOW), i)
                             if ins[j][0] == "s_mov_b64" and ops_of(ins[j][1])[1:] == ["exec"]]
                    if saved:
                        open_region(i, a[1], saved[-1])
                    else:
                        restore(i, a[1])
            # s_and / s_andn2 / s_xor into exec: loop-exit masks and the else flip; they narrow the open region
    while stack:
        close_region(hi + 1)
    out.sort(key=lambda r: r["offset"])
    body = ins[lo:hi + 1]
    top = [r for r in out if r["depth"] == 0]
    small = [r for r in top if r["size"] <= SMALL]
    lane_stores = [r for r in top if r["guard"] != "cmp" and r["store_only"]]
    tot = collections.OrderedDict(
        instructions=len(body), regions=len(out), top_level=len(top),
        branches_retained=sum(r["branch"] for r in out),
        s_cbranch_execz=sum(op == "s_cbranch_execz" for op, _ in body),
        saveexec=sum(bool(SAVEEXEC.match(op)) for op, _ in body),
        exec_writes=sum(writes_exec(op, args) for op, args in body),
        top_small=len(small), top_small_branch=sum(r["branch"] for r in small),
        top_small_branch_mask=sum(r["branch"] and r["guard"] != "cmp" for r in small),
        top_mask_store_only=len(lane_stores),
        lane_rw=sum(op.startswith(("v_readlane", "v_writelane")) for op, _ in body))
    return out, tot


def report(name, regs, tot):
    lines = [f"{name[:60]}: " + ", ".join(f"{k} {v}" for k, v in tot.items()),
             f"{'offset':>6s} {'size':>5s} {'depth':>5s} {'branch':>6s} {'guard':>10s} {'ds_w':>4s} {'ds_r':>4s} "
             f"{'valu':>5s} {'vmem':>4s} {'stores':>6s}  stage"]
    for r in regs:
        lines.append(f"{r['offset']:6d} {r['size']:5d} {r['depth']:5d} {'yes' if r['branch'] else 'no':>6s} "
                     f"{r['guard']:>10s} {r['lds_write']:4d} {r['lds_read']:4d} {r['valu']:5d} {r['vmem']:4d} "
                     f"{'only' if r['store_only'] else '':>6s}  {r['stage']}")
    per = collections.OrderedDict()
    for r in regs:
        c = per.setdefault(r["stage"], collections.Counter())
        c["regions"] += 1
        c["top"] += r["depth"] == 0
        c["branch"] += r["branch"]
        c["mask_stores"] += r["depth"] == 0 and r["guard"] != "cmp" and r["store_only"]
    lines.append(f"{'per stage':40s} {'regions':>8s} {'top':>8s} {'branch':>8s} {'mask+st':>8s}")
    for st, c in per.items():
        lines.append(f"{st[:40]:40s} {c['regions']:8d} {c['top']:8d} {c['branch']:8d} {c['mask_stores']:8d}")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="flat")
    ap.add_argument("--kernel", default="step_kernelI", help="substring of the mangled kernel name")
    ap.add_argument("--asm")
    ap.add_argument("--whole", action="store_true", help="the whole kernel instead of its largest loop body")
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--totals", action="store_true", help="the totals line only")
    ap.add_argument("-D", action="append", default=[])
    a = ap.parse_args()
    if a.asm:
        text = open(a.asm).read()
    else:
        sys.path.insert(0, ilc.ROOT)
        from open_duck_playground_amd import native
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "unit.s")
            subprocess.check_call(["hipcc"] + native.compile_flags() + ["-DDUCK_ASM_MARKS"] + [f"-D{d}" for d in a.D] +
                                  ["--cuda-device-only", "-S", "-o", out,
                                   os.path.join(native.CSRC, f"variant_{a.scene}.hip")], cwd=native.CSRC)
            text = open(out).read()
    for name, items in ilc.functions(iwc.annotate(text)).items():
        if a.kernel not in name or not name.startswith("_Z"):
            continue
        regs, tot = regions(items, a.whole)
        if a.json:
            print(json.dumps(dict(kernel=name[:60], totals=tot, regions=regs)))
        elif a.totals:
            print(f"{name[:60]}: " + ", ".join(f"{k} {v}" for k, v in tot.items()))
        else:
            print(report(name, regs, tot))


if __name__ == "__main__":
    main()
