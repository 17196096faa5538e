"""The stage, counter and doubling ids of the env kernels, read from the tables in csrc/duck_measure.h."""
import os
import re

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
_hdr = open(os.path.join(ROOT, "open_duck_playground_amd", "csrc", "duck_measure.h")).read()
ROWS = [(int(n), i, lab) for n, i, lab in re.findall(r'^\s*X\((\d+), (\w+), "([^"]*)"\)', _hdr, re.M)]
NUM = {i: n for n, i, _ in ROWS}  # identifier -> number
IDENT = {n: i for n, i, _ in ROWS}
LABEL = {n: lab for n, _, lab in ROWS}
# the stages a -DDUCK_DOUBLE=k build can run twice (DUCK_DOUBLE_TABLE): (k, label)
DOUBLES = [(int(k), lab) for k, lab in re.findall(r'^\s*D\((\d+), "([^"]*)"\)', _hdr, re.M)]
NSTAGE = int(re.search(r"^#define DUCK_NSTAGE (\d+)", _hdr, re.M).group(1))
# length in words of duck_debug_stage_cycles' buffer (include/duck.h)
CYCLES_WORDS = int(re.search(r"^#define DUCK_STAGE_CYCLES_WORDS (\d+)",
                             open(os.path.join(ROOT, "include", "duck.h")).read(), re.M).group(1))
