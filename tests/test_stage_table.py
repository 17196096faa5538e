"""The env kernels' measurement scaffolding lives in csrc/duck_measure.h: one table of stage ids that the
tools read, one exported buffer length, and no measurement switches left in the kernel headers (CPU only)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open_duck_playground_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
import stage_table as T  # noqa: E402

TOOLS = ("stage_prof.py", "lat_prof.py", "isa_stage_hist.py", "stage_pmc_summary.py")
MEASURE_FLAGS = ("DUCK_DOUBLE", "DUCK_STAGE_PROF", "DUCK_WAVE_PROF", "DUCK_LAT_PROF", "DUCK_ANY_PROF", "DUCK_ASM_MARKS",
                 "DUCK_LS_DUMP", "DUCK_AUX_LDS")
RETIRED = ("DUCK_LS_NOBREAK", "DUCK_DIAG_NO_RARE_CALLS", "DUCK_LAY_WIDE", "DUCK_LS_DFLOOR")


def _csrc_files():
    for d, _, fs in os.walk(CSRC):
        for f in fs:
            if f.endswith((".h", ".hip", ".inc")):
                yield os.path.join(d, f)


def test_table_is_consistent():
    nums = [n for n, _, _ in T.ROWS]
    ids = [i for _, i, _ in T.ROWS]
    assert len(T.ROWS) > 50
    assert len(set(nums)) == len(nums) and len(set(ids)) == len(ids)
    assert all(0 <= n < T.NSTAGE for n in nums)
    assert all(lab for _, _, lab in T.ROWS)
    dk = [k for k, _ in T.DOUBLES]
    assert len(dk) >= 19 and len(set(dk)) == len(dk) and all(k > 0 for k in dk) and all(lab for _, lab in T.DOUBLES)


def test_every_mark_in_the_kernels_is_in_the_table():
    for path in _csrc_files():
        text = open(path).read()
        for ident in re.findall(r"\bST_([A-Z0-9_]+)\b", text):
            assert ident in T.NUM, (path, ident)
        if not path.endswith("duck_measure.h"):
            # marks and counters name their stage, never a bare number
            assert not re.search(r"\b(STAGE_MARK|STAGE_ADD|STAGE_COUNT\w*)\(\s*\d", text), path
        # every doubled stage is in the table of k
        for k in re.findall(r"\bSTAGE_(?:TWICE|FRESH|AGAIN|KEEP|RESTORE)\((\w+)", text):
            assert k == "k" or int(k) in dict(T.DOUBLES), (path, k)


def test_tools_take_their_stages_from_the_table():
    for tool in TOOLS:
        text = open(os.path.join(ROOT, "tools", tool)).read()
        assert "stage_table" in text, tool
        assert not re.search(r"^NSTAGE\s*=\s*\d", text, re.M), tool
        assert "3 * 1024" not in text, tool
        # the stages a tool refers to: N["X"] / T.NUM["X"] lookups and the lists given to _group([...])
        refs = re.findall(r"""\bN(?:UM)?\[["'](\w+)["']""", text)
        for lst in re.findall(r"_group\(\[(.*?)\]\)", text, re.S):
            refs += [s.strip() for s in re.findall(r'"([^"]+)"', lst)]
        for r in refs:
            assert r in T.NUM, (tool, r)
    assert "_group([" in open(os.path.join(ROOT, "tools", "stage_prof.py")).read()


def test_stage_cycles_buffer_length():
    from open_duck_playground_amd.cabi import STAGE_CYCLES_WORDS
    assert T.CYCLES_WORDS == STAGE_CYCLES_WORDS == T.NSTAGE + 3 * 1024
    hdr = open(os.path.join(CSRC, "duck_measure.h")).read()
    assert "static_assert(DUCK_STAGE_CYCLES_WORDS == DUCK_NSTAGE + 3 * 1024" in hdr


def test_measurement_switches_only_in_duck_measure_h():
    cond = re.compile(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b(.*)$", re.M)
    for path in _csrc_files():
        text = open(path).read()
        for name in RETIRED:
            assert name not in text, (path, name)
        if path.endswith("duck_measure.h"):
            continue
        for line in cond.findall(text):
            for flag in MEASURE_FLAGS:
                assert not re.search(rf"\b{flag}\b", line), (path, line.strip())
