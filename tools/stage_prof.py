#!/usr/bin/env python3
"""Per-stage cycle breakdown of step_kernel (needs a -DDUCK_STAGE_PROF build in DUCK_LIB).

Counters are wave-0 clock64 deltas summed over workgroups; printed per substep per wave.
The top-level stages (TOP) partition a substep. Sub-stage counters (SUB) measure from the start of
their parent stage. Numbers and labels come from csrc/duck_measure.h (stage_table.py).
"""
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from open_duck_playground_amd import native  # noqa: E402
from open_duck_playground_amd.joystick import Joystick, wrap_for_brax_training  # noqa: E402

import stage_table as T  # noqa: E402

# how this tool groups the stages (numbers and labels: csrc/duck_measure.h); "  " indents a sub-stage
_group = lambda ids: {T.NUM[i.strip()]: i[:len(i) - len(i.lstrip())] + T.LABEL[T.NUM[i.strip()]] for i in ids}
TOP = _group(["KINEMATICS", "COM_POS", "RNE", "CRB", "SMOOTH", "COLLISION", "MAKE_ROWS", "LOAD_COLS", "SMOOTH_ACC", "SOLVE",
              "SENSORS_EULER"])
SUB = _group(["KIN_LOCAL", "RNE_A", "RNE_B", "RNE_LIMB", "RNE_ROOT", "CRB_SUMS", "COLLISION_FLOOR", "WARM_PRODUCTS",
              "WARM_SELECT", "NEWTON_DIR", "  NEWTON_GRAD", "  NEWTON_JDJ", "  NEWTON_FACTOR", "NEWTON_SPARSE",
              "SEARCH_PRODUCTS", "LINESEARCH", "HF_SCREEN", "HF_QUEUE", "HF_SLOTS", "  HFQ_DESC", "  HFQ_SAT", "  HFQ_GATHER",
              "    SAT_VERTICAL", "    SAT_PASS1", "    SAT_PASS2"])
ENV = _group(["ENV_HOT_LOAD", "ENV_RNG", "ENV_PRE", "ENV_CONTACTS_OBS", "ENV_TERM", "ENV_OBS_STORE", "ENV_HOT_STORE"])
NSTAGE = T.NSTAGE
N = T.NUM


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    rand = "--random" in sys.argv  # bench.py's U(-1,1) actions (more contacts than zero actions)
    task = next((a.split("=", 1)[1] for a in sys.argv if a.startswith("--task=")), "flat_terrain")
    env = wrap_for_brax_training(Joystick(task, num_envs=n, device="cuda:0", use_imitation=False),
                                 episode_length=1000)
    st = env.reset(rng=0)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1234)
    pool = [torch.rand(n, env.action_size, device="cuda:0", generator=g) * 2 - 1 for _ in range(8)] if rand else \
        [torch.zeros(n, env.action_size, device="cuda:0")]
    warm = next((int(a.split("=", 1)[1]) for a in sys.argv if a.startswith("--warm=")), 20)
    for i in range(warm):
        st = env.step(st, pool[i % len(pool)], inplace=True)
    torch.cuda.synchronize()
    buf = (C.c_ulonglong * T.CYCLES_WORDS)()
    lib = native.lib()
    lib.duck_debug_stage_cycles(env._sim, buf, 1)
    steps = next((int(a.split("=", 1)[1]) for a in sys.argv if a.startswith("--steps=")), 5)
    for i in range(steps):
        st = env.step(st, pool[(warm + i) % len(pool)], inplace=True)
    torch.cuda.synchronize()
    lib.duck_debug_stage_cycles(env._sim, buf, 1)
    nwg = (n + 15) // 16
    per_sub = lambda k: buf[k] / (nwg * steps * 10)
    tot = sum(buf[k] for k in TOP) or 1  # (0 in a -DDUCK_WAVE_PROF build: wave times only)
    for k, name in TOP.items():
        print(f"{name:28s} {per_sub(k):10.0f} cycles/substep/wave  {100 * buf[k] / tot:5.1f}%")
    for k, name in SUB.items():
        print(f"{name:28s} {per_sub(k):10.0f}")
    per = lambda k: buf[k] / (nwg * steps)
    for k, name in ENV.items():
        print(f"{name:28s} {per(k):10.0f} cycles/env-step/wave")
    import numpy as np
    w = np.array([buf[NSTAGE + i] for i in range(min(1024, 4 * nwg))], dtype=np.float64)
    w = w[w > 0]
    if len(w):
        print(f"{'wave cycles (last launch)':28s} mean {w.mean():.0f}  p50 {np.median(w):.0f}  p99 {np.quantile(w, 0.99):.0f}  "
              f"max {w.max():.0f}  max/mean {w.max() / w.mean():.3f}")
        if len(w) == 4 * nwg and "--waves" in sys.argv:
            wg = w.reshape(-1, 4)
            print("  per-workgroup max/min spread: mean %.3f" % (wg.max(1) / wg.min(1)).mean())
            print("  per-XCD (blockIdx % 8) mean wave cycles:", [int(wg[x::8].mean()) for x in range(8)])
            print("  per wave-in-workgroup mean:", [int(wg[:, k].mean()) for k in range(4)])
            print("  slowest workgroups:", [int(x) for x in np.argsort(wg.max(1))[-8:]])
            t0 = np.array([buf[NSTAGE + 1024 + i] for i in range(4 * nwg)], dtype=np.float64).reshape(-1, 4)
            t1 = np.array([buf[NSTAGE + 2048 + i] for i in range(4 * nwg)], dtype=np.float64).reshape(-1, 4)
            base = t0.min()
            us = lambda a: (a - base) / 100.0  # s_memrealtime: 100 MHz
            print("  wall clock per XCD (us from the first wave's start): start mean/max, end mean/max")
            for x in range(8):
                print(f"    XCD {x}: start {us(t0[x::8]).mean():7.1f} {us(t0[x::8]).max():7.1f}  "
                      f"end {us(t1[x::8]).mean():7.1f} {us(t1[x::8]).max():7.1f}  "
                      f"duration mean {((t1[x::8] - t0[x::8]) / 100).mean():7.1f}")
            print(f"  launch span (first start to last end): {us(t1).max():.1f} us")
    print(f"{'dense Newton fallbacks':28s} {buf[N['N_DENSE_FALLBACK']] / steps:10.1f} per env-step (all {n} envs)")
    print(f"{'foot/foot SAT runs':28s} {buf[N['N_FOOT_SAT']] / steps:10.1f} per env-step (all {n} envs)")
    if buf[N['N_HF_SURVIVORS']]:
        print(f"{'hfield survivors':28s} {buf[N['N_HF_SURVIVORS']] / (nwg * steps * 10):10.2f} per substep (wave 0 of each workgroup: 8 feet)")
        print(f"{'hfield queue rounds':28s} {buf[N['N_HF_ROUNDS']] / (nwg * steps * 10):10.2f} per substep (wave 0)")
        print(f"{'hfield pass-2 iterations':28s} {buf[N['N_HF_PASS2_ITERS']] / (nwg * steps * 10):10.2f} per substep (wave 0: the most crossing pairs of a lane)")
        print(f"{'hfield crossing pairs':28s} {buf[N['N_HF_PAIRS']] / (nwg * steps * 10):10.2f} per substep (wave 0: all survivors)")
        print(f"{'hfield crossing edges':28s} {buf[N['N_HF_EDGES']] / (nwg * steps * 10):10.2f} per substep (wave 0: hull edges crossing in any survivor)")
        hist = [buf[N['N_HF_SURV_LE21']], buf[N['N_HF_SURV_LE32']], buf[N['N_HF_SURV_LE42']], buf[N['N_HF_SURV_LE64']],
                buf[N['N_HF_SURV_GT64']]]
        if sum(hist):
            print(f"{'hfield survivors per wave':28s} " + ", ".join(
                f"{lab}: {100 * v / sum(hist):.1f} %" for lab, v in zip(("<=21", "22-32", "33-42", "43-64", ">64"), hist)))
    outside = per(N['MODEL_COPY']) + sum(per(k) for k in ENV)
    kern = outside + tot / (nwg * steps)
    if per(N['MODEL_COPY']) == 0:
        return
    if buf[N['N_LS_SEARCHES']] > 0:
        # line search (wave 0 of each workgroup): iterations the wave ran vs its teams needed
        print(f"{'line search iterations':28s} per team {buf[N['N_LS_TEAM_ITERS']] / buf[N['N_LS_SEARCHES']]:.2f}, per wave {4 * buf[N['N_LS_WAVE_ITERS']] / buf[N['N_LS_SEARCHES']]:.2f} "
              f"({buf[N['N_LS_SEARCHES']] / (nwg * steps * 10) / 4:.2f} searches per team and substep)")
    print(f"{'kernel (per env-step)':28s} {kern:10.0f} cycles/env-step/wave (sum of the marked sections)")
    print(f"{'  model-table copy':28s} {per(N['MODEL_COPY']):10.0f}  {100 * per(N['MODEL_COPY']) / kern:5.1f}%")
    print(f"{'  10 substeps':28s} {tot / (nwg * steps):10.0f}  {100 * tot / (nwg * steps) / kern:5.1f}%")
    print(f"{'  env code outside':28s} {outside - per(N['MODEL_COPY']):10.0f}  {100 * (outside - per(N['MODEL_COPY'])) / kern:5.1f}%")


if __name__ == "__main__":
    main()
