#!/usr/bin/env python3
"""How well a kernel's LDS waits are covered, from hipcc -S output (CPU only).

The step kernels run one wave per SIMD, so an LDS round trip is hidden only by the wave's own
instructions between the load and the s_waitcnt that retires it. For the largest loop body of a kernel
(tools/isa_loop_count.py's body: the substep loop) this prints
  - the basic blocks: count and size histogram (a block starts at a label and after a branch);
  - the exec-masked regions (s_*_saveexec, s_and / s_andn2 into exec, v_cmpx) and the wave barriers
    ("; wave barrier" comments: a TSYNC() is one);
  - for every s_waitcnt with an lgkmcnt: the number of VALU instructions between the wait and the youngest
    ds_read it retires, binned 0-3 / 4-11 / 12-23 / 24+ / "earlier" (the wait retires no load of its own
    block: the load was issued in an earlier block, or only stores are outstanding);
  - the same bins per stage, by the "; STAGE_MARK ST_x" comments of a -DDUCK_ASM_MARKS build (the
    region that ends at mark x carries x's name, as in tools/isa_stage_hist.py).
LDS operations complete in issue order, so a wait for lgkmcnt(N) retires every outstanding operation
but the youngest N; scalar loads share the counter and are counted as outstanding operations.

usage: python tools/isa_wait_cover.py [--scene flat] [--kernel step_kernelI] [--asm FILE] [--whole]
                                      [--json] [-D DEFINE ...]
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

BINS = ["0-3", "4-11", "12-23", "24+", "earlier"]
SIZES = [("1-9", 1, 9), ("10-24", 10, 24), ("25-99", 25, 99), ("100+", 100, 1 << 30)]
MARK, WBAR = ".Lmark.", ".Lwavebarrier."
TERM = ("s_branch", "s_cbranch", "s_endpgm", "s_setpc", "s_swappc")
EXEC_OPEN = re.compile(r"^(s_\w+_saveexec_b64\b|v_cmpx_)")


def annotate(text):
    """The stage marks and wave barriers (assembly comments, which the parser drops) as local labels."""
    out, n = [], 0
    for line in text.splitlines():
        m = re.match(r"\s*;\s*STAGE_MARK (\w+)", line)
        if m:
            line = f"{MARK}{m.group(1)}.{n}:"
        elif re.match(r"\s*;\s*wave barrier", line):
            line = f"{WBAR}{n}:"
        n += 1
        out.append(line)
    return "\n".join(out)


def bin_of(nvalu):
    return BINS[0] if nvalu <= 3 else BINS[1] if nvalu <= 11 else BINS[2] if nvalu <= 23 else BINS[3]


def lgkm_of(args):
    m = re.search(r"lgkmcnt\((\d+)\)", args)
    if m:
        return int(m.group(1))
    if re.fullmatch(r"\s*(0x[0-9a-fA-F]+|\d+)\s*", args or ""):  # raw immediate: lgkmcnt is bits 11:8
        return (int(args, 0) >> 8) & 0xF
    return None


def body_range(items):
    """(first, last) instruction index of the longest backward branch's loop, as isa_loop_count.loop_body"""
    pos, k, ins = {}, 0, []
    for kind, a, b in items:
        if kind == "label":
            pos[a] = k
        else:
            ins.append((a, b))
            k += 1
    best = (0, 0, len(ins) - 1)
    for i, (op, args) in enumerate(ins):
        if op.startswith(("s_cbranch", "s_branch")):
            t = pos.get(args.strip())
            if t is not None and t <= i and i - t > best[0]:
                best = (i - t, t, i)
    return best[1], best[2]


def census(items, whole=False):
    """items: isa_loop_count.functions()'s list of one kernel, from annotate()d text"""
    lo, hi = (0, sum(k == "ins" for k, _, _ in items) - 1) if whole else body_range(items)
    # the mark that closes each instruction's region
    stage_at, pending, k = {}, [], 0
    for kind, a, _ in items:
        if kind == "ins":
            pending.append(k)
            k += 1
        elif a.startswith(MARK):
            for p in pending:
                stage_at[p] = a[len(MARK):].rsplit(".", 1)[0]
            pending = []
    blocks, sizes, cur = 0, [], 0
    exec_regions = barriers = 0
    waits = []  # (stage, bin)
    queue, nvalu, k, new_block = [], 0, 0, True  # queue: (is_read, VALU count at issue) of the block's lgkm ops
    for kind, a, b in items:
        inside = lo <= k <= hi
        if kind == "label":
            if a.startswith(WBAR):
                barriers += inside
            elif not a.startswith(MARK):
                new_block = True
            continue
        if inside:
            if new_block:
                if cur:
                    sizes.append(cur)
                cur, queue, nvalu = 0, [], 0
            cur += 1
            op = a
            if EXEC_OPEN.match(op) or (op in ("s_and_b64", "s_andn2_b64") and b.split(",")[0].strip() == "exec"):
                exec_regions += 1
            if op.startswith("ds_") or op.startswith(("s_load_", "s_buffer_load_")):
                queue.append((op.startswith("ds_read") or op.startswith("ds_load"), nvalu))
            elif op.startswith("v_"):
                nvalu += 1
            elif op == "s_waitcnt":
                n = lgkm_of(b)
                if n is not None:
                    done, queue = (queue[:len(queue) - n], queue[len(queue) - n:]) if n < len(queue) else ([], queue)
                    reads = [v for r, v in done if r]
                    waits.append((stage_at.get(k, "(after last mark)"), bin_of(nvalu - reads[-1]) if reads else BINS[4]))
        new_block = a.startswith(TERM)
        k += 1
    if cur:
        sizes.append(cur)
    per_stage = collections.OrderedDict()
    for st, bn in waits:
        per_stage.setdefault(st, collections.Counter())[bn] += 1
    tot = collections.Counter(bn for _, bn in waits)
    return {"instructions": hi - lo + 1, "blocks": len(sizes),
            "block_sizes": {name: sum(a <= s <= b for s in sizes) for name, a, b in SIZES},
            "exec_regions": exec_regions, "wave_barriers": barriers, "lgkm_waits": len(waits),
            "bins": {bn: tot[bn] for bn in BINS},
            "stages": {st: {bn: c[bn] for bn in BINS} for st, c in per_stage.items()}}


def report(name, c):
    lines = [f"{name[:60]}: {c['instructions']} instructions in {c['blocks']} basic blocks ("
             + ", ".join(f"{k}: {v}" for k, v in c["block_sizes"].items()) + ")",
             f"exec-masked regions {c['exec_regions']}, wave barriers {c['wave_barriers']}, "
             f"s_waitcnt lgkmcnt {c['lgkm_waits']}",
             f"{'VALU between youngest ds_read and wait':40s} " + " ".join(f"{b:>8s}" for b in BINS)]
    for st, bins in list(c["stages"].items()) + [("total", c["bins"])]:
        lines.append(f"{st[:40]:40s} " + " ".join(f"{bins[b]:8d}" for b in BINS))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", default="flat")
    ap.add_argument("--kernel", default="step_kernelI", help="substring of the mangled kernel name")
    ap.add_argument("--asm")
    ap.add_argument("--whole", action="store_true", help="the whole kernel instead of its largest loop body")
    ap.add_argument("--json", action="store_true")
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
    for name, items in ilc.functions(annotate(text)).items():
        if a.kernel not in name or not name.startswith("_Z"):
            continue
        c = census(items, a.whole)
        print(json.dumps(dict(kernel=name[:60], **c)) if a.json else report(name, c))


if __name__ == "__main__":
    main()
