#!/usr/bin/env python3
"""Diff the env's LDS slice after one forward between two inlined copies of the substep.

physics_kernel inlines the substep twice: nsub=0 (mjx.forward) and the nsub>=1 loop. From the
same state (zero warm start) both compute the same forward, so the nsub=0 copy is an exact
reference for the loop copy. Needs a library built with -DDUCK_AUX_LDS (write_aux appends the
whole slice). Prints, per Lay field in pipeline order, the envs that differ and by how much."""
import os
import re
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
from open_duck_playground_amd.joystick import Joystick  # noqa: E402
from tests.helpers import random_states  # noqa: E402

task = sys.argv[1] if len(sys.argv) > 1 else "rough_terrain_backlash"
seed = int(sys.argv[2]) if len(sys.argv) > 2 else 2
n = 512
gen = os.path.join(os.path.dirname(__file__), "..", "open_duck_playground_amd", "csrc", "generated",
                   {"flat_terrain": "duck_model_flat.h", "flat_terrain_backlash": "duck_model_backlash.h",
                    "rough_terrain": "duck_model_rough.h",
                    "rough_terrain_backlash": "duck_model_rough_backlash.h"}[task])
txt = open(gen).read()
C = {k: int(v) for k, v in re.findall(r"\b(NB|NQ|NV|NU|NM|MAXCHAIN|NSENSORDATA|NPAIR|NFRIC|NLIM|NHE|NHF|FLOOR_TYPE|NBLOB|B_HFACE|B_HEND) = (\d+)", txt)}
NB, NQ, NV, NU, NM = C["NB"], C["NQ"], C["NV"], C["NU"], C["NM"]
NCON = 4 * C["NPAIR"]
R_CON = C["NFRIC"] + C["NLIM"]
NROW = R_CON + 4 * NCON
# Lay::HSZ: the scratch in front of the rows, sized for its largest user
need = max(12 * NB + 6 * NV, 6 * (C["NHE"] + C["NHF"]), 3 + 28 * 16 if C["FLOOR_TYPE"] == 1 else 0, 86 + 9 * NU)
HSZ = (max(need - 4 * NROW - C["NLIM"], 0) + 3) // 4 * 4


def lay_fields(al, wide):
    """LayT<Md, AL, WIDE> (csrc/duck_physics.h): the fields in slice order, padding as "pad" entries."""
    out, pos = [], [0]

    def up(a):
        pad = -pos[0] % min(al, a)
        if pad:
            out.append(("pad", pad))
            pos[0] += pad

    def put(name, k, a=1, shift=0):
        pos[0] += shift
        up(a)
        pos[0] -= shift
        out.append((name, k))
        pos[0] += k

    xps, xms, crs, cfs = (4, 10, 4, 10) if wide else (3, 9, 3, 9)
    put("XQ", 4 * NB), put("XMAT", xms * NB), put("XPOS", xps * NB, 4), put("CIN", 10 * NB, 4), put("CVEL", 6 * NB, 4)
    put("CDOF", 6 * NV, 4), put("M", NM, 4), put("MZERO", 1), put("CDD1", 18, 2), put("COM", 3, 4), put("IMUR", 3)
    put("OCON", 2), put("FOOTZ", 2), put("FLAGS", 2), put("H", HSZ, 4)
    for r in ("JA", "JV", "RD", "AREF"):
        put(r, NROW, 4, R_CON)  # the contact rows (from R_CON on) start on a 4-float boundary
    put("LSGN", C["NLIM"], 2), put("CR", crs * NCON, 4), put("CFR", cfs * NCON, 4), put("CDIST", NCON, 4)
    put("AF", NU, 2), put("SENS", C["NSENSORDATA"], 2)
    for name, k in (("QPOS", NQ), ("QVEL", NV), ("WARM", NV), ("CTRL", NU), ("QACC", NV), ("QSM", NV), ("FSM", NV),
                    ("SRCH", NV), ("GRAD", NV), ("MA", NV), ("DMASS", NB), ("DIPOS", 3), ("DARM", NV), ("DFRIC", NV),
                    ("DQ0", NQ), ("DKP", NU)):
        put(name, k)
    up(4)
    return out, pos[0]


def lay_keeps(total):
    """duck_physics.h lay_keeps: what stays in LDS next to 16 slices of `total` words"""
    W, tab = 160 * 1024 // 4, 16 * (((total + 32 + 15) // 32) * 32 + 16)
    nht = max(C.get("B_HEND", 0) - C.get("B_HFACE", 0), 0)
    tabl = tab + C["NBLOB"] <= W
    htl = not tabl and nht > 0 and tab + nht <= W
    es = tab + (C["NBLOB"] if tabl else (nht if htl else 0))
    esl = es + 16 * ((NQ + 2 * NV + 8 * NU + 77 + 64) | 1) <= W
    return -1 if es > W else tabl + 2 * htl + 4 * esl


# Lay<Md>: the first rule whose slices keep in LDS what the packed ones keep (lay_rule)
keep = lay_keeps(lay_fields(1, False)[1])
al, wide = next((a, w) for w in (True, False) for a in (4, 2, 1) if lay_keeps(lay_fields(a, w)[1]) == keep)
fields = lay_fields(al, wide)[0] + [("SINK", 32)]
total = sum(k for _, k in fields)

env = Joystick(task, num_envs=1, device="cuda:0", use_imitation=False)
m = env.mj_model
qpos, qvel, ctrl = random_states(m, n, seed)
T = lambda a: torch.tensor(np.ascontiguousarray(a.T), dtype=torch.float32, device="cuda:0")
outs = []
for nsub in (0, 1):
    tq, tv, tw, tc = T(qpos), T(qvel), T(np.zeros((n, m.nv))), T(ctrl)
    aux = torch.zeros(env.aux_size() * n, dtype=torch.float32, device="cuda:0").view(-1, n)
    env.physics_step(tq, tv, tw, tc, nsub, aux)
    torch.cuda.synchronize()
    outs.append(aux.cpu().numpy()[-total:].T.astype(np.float64))
a, b = outs
os.makedirs("gpurun_out", exist_ok=True)
np.savez_compressed(f"gpurun_out/diag_lds_{task}_{seed}_{os.path.basename(os.environ.get('DUCK_LIB', 'libduck.so'))}.npz",
                    a=a, b=b, qpos=qpos, qvel=qvel, ctrl=ctrl)
o = 0
for name, k in fields:
    x, y = a[:, o:o + k], b[:, o:o + k]
    o += k
    if name in ("QPOS", "QVEL", "pad"):
        continue  # padding is never written; the loop copy integrates after write_aux? (aux is written before euler)
    d = np.abs(x - y) / (1 + np.abs(x))
    d[~(np.isfinite(x) & np.isfinite(y) & (np.abs(x) < 1e20))] = 0.0  # never-written slots (world/floor bodies)
    bad = np.where(d.max(axis=1) > 1e-5)[0]
    if len(bad):
        cols = np.argsort(-d[bad].max(axis=0))[:6]
        print(f"{name:6s} {len(bad):4d} envs differ; worst {d.max():.3e}; envs {bad[:12].tolist()} cols {cols.tolist()}",
              flush=True)
    else:
        print(f"{name:6s} identical (<=1e-5)", flush=True)
