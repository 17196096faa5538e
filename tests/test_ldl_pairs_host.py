"""The compile-time pairing table of the register LDL' row updates (csrc/duck_ldlpairs.h) against the dof tree.

Pivot k of the factorization updates every ancestor row i of k in the column sets that reach it (16 s <= i);
rows 2m, 2m + 1 that are both updated in a set go as one packed FMA. A host C++ program
(tests/ldl_pairs_main.cpp, its own main, no GPU) includes each generated model header -- the four shipped
scenes and the header codegen writes for tests/golden/models/flat_terrain_head_last.npz -- and prints, per
pivot and set, the low rows and high rows of the pairs and the rows updated alone. Checked here against an
independent walk of dof_parentid:
  * every pair is two ancestors 2m, 2m + 1 of the pivot, both inside the set's range;
  * no row is updated twice and none is dropped: pairs plus singles are the scalar code's update list;
  * no two adjacent rows 2m, 2m + 1 are both left as singles (the table pairs all it can).
One edited tree that no shipped scene has (a branch inside a limb, a limb across the set boundary) goes
through the same checks.
"""

import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")
GEN = os.path.join(CSRC, "generated")
SRC = os.path.join(ROOT, "tests", "ldl_pairs_main.cpp")
VARIANTS = sorted(f[len("duck_model_"):-2] for f in os.listdir(GEN) if f.startswith("duck_model_") and f.endswith(".h"))
TEAM = 16


def _compiler():
    for cc in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++"):
        p = shutil.which(cc)
        if p:
            return p
    raise RuntimeError("no host C++ compiler")


def _table(tmp_path, header=None, struct=None):
    """(nv, parent, {(k, s): (lo, hi, single)}) as the program built on `header` prints it."""
    exe = str(tmp_path / "ldl_pairs")
    cmd = [_compiler(), "-std=c++17", "-O0", "-I" + CSRC, "-o", exe, SRC]
    if header:
        cmd += ["-D__device__=", "-D__forceinline__=inline", f'-DMODEL_HEADER="{header}"', f"-DMODEL={struct}"]
    subprocess.check_call(cmd)
    nv, on, parent, tab = None, None, None, {}
    for line in subprocess.check_output([exe], text=True).splitlines():
        w = line.split()
        if w[0] == "NV":
            nv, on = int(w[1]), int(w[5])
        elif w[0] == "parent":
            parent = [int(x) for x in w[1:]]
        elif w[0] == "pivot":
            a, b, c = w.index("lo"), w.index("hi"), w.index("single")
            tab[(int(w[1]), int(w[3]))] = ([int(x) for x in w[a + 1:b]], [int(x) for x in w[b + 1:c]],
                                           [int(x) for x in w[c + 1:]])
    assert on == 1, "the shipped build takes the packed form"
    return nv, parent, tab


def _ancestors(parent, d):
    out, j = [], parent[d]
    while j >= 0:
        out.append(j)
        j = parent[j]
    return out


def _check(nv, parent, tab):
    """Returns (pairs, updates) summed over the pivots."""
    nc = (nv + TEAM - 1) // TEAM
    assert len(tab) == nv * nc and len(parent) == nv
    npair = nupd = 0
    for k in range(nv):
        anc = _ancestors(parent, k)
        for s in range(nc):
            lo, hi, single = tab[(k, s)]
            want = sorted(i for i in anc if TEAM * s <= i)  # the scalar code's update list
            assert hi == [i + 1 for i in lo], (k, s)
            for i in lo:
                assert i % 2 == 0 and i in anc and i + 1 in anc and TEAM * s <= i, (k, s, i)
            got = sorted(lo + hi + single)
            assert got == want, f"pivot {k} set {s}: updated {got}, the tree says {want}"
            assert len(set(got)) == len(got)
            assert not any(i % 2 == 0 and i + 1 in single for i in single), (k, s, single)
            npair += len(lo)
            nupd += len(want)
    return npair, nupd


@pytest.mark.parametrize("variant", VARIANTS)
def test_pairs_match_tree(variant, tmp_path):
    from open_duck_playground_amd import codegen, constants
    from open_duck_playground_amd.mjcf import Model
    nv, parent, tab = _table(tmp_path, f"generated/duck_model_{variant}.h", f"DuckModel_{variant}")
    m = Model.load(constants.task_to_xml(dict(codegen.DEFAULT_VARIANTS)[variant]))
    assert nv == m.nv and parent == [int(x) for x in np.asarray(m.dof_parentid)], "the header's tree is mjcf.py's"
    npair, nupd = _check(nv, parent, tab)
    print(f"{variant}: {npair} packed + {nupd - 2 * npair} scalar FMAs for {nupd} row updates")
    assert npair > 0


def test_flat_pair_count(tmp_path):
    """Flat scene: the free joint's rows 0-5 are three pairs under every limb pivot, a limb's own rows pair
    where they start at an even dof; the right leg's rows 16-19 are the only ones set 1 reaches."""
    nv, parent, tab = _table(tmp_path, "generated/duck_model_flat.h", "DuckModel_flat")
    npair, nupd = _check(nv, parent, tab)
    for k in range(6, nv):
        assert tab[(k, 0)][0][:3] == [0, 2, 4]
    assert all(i >= TEAM for (k, s), v in tab.items() if s == 1 for i in v[0] + v[1] + v[2])
    assert tab[(19, 1)] == ([16], [17], [18])


def test_head_last_tree(tmp_path):
    from open_duck_playground_amd import codegen
    from open_duck_playground_amd.mjcf import Model
    from tests.kat_checks import model_path
    m = Model.load(model_path("flat_terrain_head_last"))
    (tmp_path / "duck_model_hl.h").write_text(codegen.model_header(m, "hl"))
    nv, parent, tab = _table(tmp_path, str(tmp_path / "duck_model_hl.h"), "DuckModel_hl")
    assert parent == [int(x) for x in np.asarray(m.dof_parentid)]
    npair, _ = _check(nv, parent, tab)
    # the head limb (dofs 16-19, parent dof 5) is set 1's: pivot 19 pairs rows 16, 17 in both sets (set 0's
    # columns 0-5 reach every row) and rows 0-5 in set 0; the right leg (dofs 11-15) is not among its ancestors
    assert tab[(19, 1)] == ([16], [17], [18]) and tab[(19, 0)] == ([0, 2, 4, 16], [1, 3, 5, 17], [18])
    assert npair > 0


def test_edited_tree(tmp_path):
    nv, parent, tab = _table(tmp_path)
    assert nv == 19
    _check(nv, parent, tab)
    # dof 9 hangs on dof 6: its ancestors 0-6 give three pairs and row 6 alone
    assert tab[(9, 0)] == ([0, 2, 4], [1, 3, 5], [6])
    # the long limb 10-18 on dof 5: pivot 18's rows 10-15 pair in set 0; set 1 reaches rows 16, 17 only
    assert tab[(18, 0)] == ([0, 2, 4, 10, 12, 14, 16], [1, 3, 5, 11, 13, 15, 17], [])
    assert tab[(18, 1)] == ([16], [17], [])
    assert tab[(17, 1)] == ([], [], [16])
