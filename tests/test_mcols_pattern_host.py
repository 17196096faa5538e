"""The compile-time pattern table of M's register columns (csrc/duck_mcols.h) against the dof tree and B_MADR.

A host C++ program (tests/mcols_pattern_main.cpp, its own main, no GPU) includes each generated model header
and prints, per row r and column set s, the lanes that take the descendant form, the ancestor form and zero,
the flag "zero on every lane" that the throughput kernel's M x relies on, and the header's M address table.
Checked here against the tree (an independent walk of dof_parentid) and the pattern of B_MADR:
  * every (r, c) with an M address gets exactly one form, the descendant form iff c <= r;
  * every other entry of a column of M is zero, and so is every lane past NV;
  * rows flagged all-zero are zero for every valid lane, and no other row is;
  * the descendant lanes lie at or below the row's threshold lane, the ancestor lanes above it.
One edited tree that no shipped scene has (a branch inside a limb, a limb across the set boundary) goes
through the same checks against the tree alone.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")
GEN = os.path.join(CSRC, "generated")
SRC = os.path.join(ROOT, "tests", "mcols_pattern_main.cpp")
VARIANTS = sorted(f[len("duck_model_"):-2] for f in os.listdir(GEN) if f.startswith("duck_model_") and f.endswith(".h"))
TEAM = 16


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(cc)
        if p:
            return p
    raise RuntimeError("no host C++ compiler")


def _table(tmp_path, variant):
    exe = str(tmp_path / f"mcols_{variant or 'edited'}")
    cmd = [_compiler(), "-std=c++17", "-O0", "-I" + CSRC, "-o", exe, SRC]
    if variant:
        cmd += ["-D__device__=", "-D__forceinline__=inline", f'-DMODEL_HEADER="generated/duck_model_{variant}.h"',
                f"-DMODEL=DuckModel_{variant}"]
    subprocess.check_call(cmd)
    rows, madr, parent, nv = {}, {}, None, None
    for line in subprocess.check_output([exe], text=True).splitlines():
        w = line.split()
        if w[0] == "NV":
            nv = int(w[1])
        elif w[0] == "parent":
            parent = [int(x) for x in w[1:]]
        elif w[0] == "row":
            v = dict(zip(w[4::2], (int(x) for x in w[5::2])))
            rows[(int(w[1]), int(w[3]))] = v
        elif w[0] == "madr":
            madr[int(w[1])] = [int(x) for x in w[2:]]
    return nv, parent, rows, madr


def _ancestors(parent, d):
    out, j = set(), parent[d]
    while j >= 0:
        out.add(j)
        j = parent[j]
    return out


def _check(nv, parent, rows, madr):
    nc = (nv + TEAM - 1) // TEAM
    assert len(rows) == nv * nc and len(parent) == nv
    related = np.zeros((nv, nv), bool)
    for d in range(nv):
        related[d, d] = True
        for a in _ancestors(parent, d):
            related[d, a] = related[a, d] = True
    if madr:
        A = np.array([madr[i] for i in range(nv)])
        assert ((A >= 0) == related).all(), "B_MADR's pattern is the tree's"
    for (r, s), v in rows.items():
        assert v["d"] & v["a"] == 0 and v["d"] & v["z"] == 0 and v["a"] & v["z"] == 0
        for lane in range(TEAM):
            c, bit = TEAM * s + lane, 1 << lane
            if c >= nv:
                assert not (v["d"] | v["a"] | v["z"]) & bit, "a column past NV takes no form"
                continue
            if related[r, c]:
                assert bool(v["d"] & bit) == (c <= r) and bool(v["a"] & bit) == (c > r) and not v["z"] & bit
                assert (lane <= v["thresh"]) == (c <= r)
            else:
                assert v["z"] & bit and not (v["d"] | v["a"]) & bit
        valid = [TEAM * s + lane for lane in range(TEAM) if TEAM * s + lane < nv]
        assert bool(v["zero"]) == (not related[r, valid].any())
        assert v["depth"] == len(_ancestors(parent, r))


@pytest.mark.parametrize("variant", VARIANTS)
def test_pattern_matches_tree_and_madr(variant, tmp_path):
    from open_duck_playground_amd import codegen, constants
    from open_duck_playground_amd.mjcf import Model
    nv, parent, rows, madr = _table(tmp_path, variant)
    task = dict(codegen.DEFAULT_VARIANTS)[variant]
    m = Model.load(constants.task_to_xml(task))
    assert nv == m.nv and parent == [int(x) for x in np.asarray(m.dof_parentid)], "the header's tree is mjcf.py's"
    assert len(madr) == nv
    _check(nv, parent, rows, madr)


def test_flat_zero_rows():
    """The rows the flat scenes' M x skips: rows 6-14 (left leg, head) of set 1 (the right leg's dofs 16-19)."""
    import tempfile
    import pathlib
    with tempfile.TemporaryDirectory() as t:
        nv, parent, rows, _ = _table(pathlib.Path(t), "flat")
    assert sorted(k for k, v in rows.items() if v["zero"]) == [(r, 1) for r in range(6, 15)]


def test_edited_tree(tmp_path):
    nv, parent, rows, madr = _table(tmp_path, None)
    assert nv == 19 and not madr
    _check(nv, parent, rows, madr)
    # the 1-dof limb on dof 6 (dof 9) is unrelated to the rest of its parent limb and to the long limb
    assert rows[(9, 0)]["z"] == (1 << 7) | (1 << 8) | sum(1 << l for l in range(10, 16))
    assert rows[(9, 1)]["zero"] == 1 and rows[(7, 1)]["zero"] == 1 and rows[(12, 1)]["zero"] == 0
