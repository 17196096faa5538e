"""tools/isa_wait_cover.py on a short synthetic assembly text: blocks, wait bins, stage attribution."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_wait_cover as W  # noqa: E402

VALU = "\tv_add_f32_e32 v1, v2, v3\n"

# one kernel: a prologue, then a loop (the body) of four blocks in three stages
ASM = (
    "\t.text\n"
    "_Z6kernelIiEvv:                         ; @kernel\n"
    "\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n"
    "\ts_waitcnt lgkmcnt(0)\n"                       # outside the body: not counted
    ".LBB0_1:                                ; the loop\n"
    # stage A: a read waited for after 2 VALU (0-3); then an index -> data chain, each link exposed
    "\tds_read_b32 v4, v0\n" + 2 * VALU +
    "\ts_waitcnt lgkmcnt(0)\n"
    "\tds_read_b32 v5, v4\n"
    "\ts_waitcnt lgkmcnt(0)\n"
    "\t;;#ASMSTART\n\t; STAGE_MARK ST_KINEMATICS\n\t;;#ASMEND\n"
    # stage B: two reads, five VALU, a wait for the older one only (lgkmcnt(1)): 5 VALU after it -> 4-11;
    # then 20 more and the wait for the younger: 25 -> 24+. A store after the reads does not hide them:
    # lgkmcnt(1) with read, read, write outstanding retires both reads, the younger 12 VALU back -> 12-23
    "\tds_read_b32 v6, v0\n"
    "\tds_read_b32 v7, v0 offset:4\n" + 5 * VALU +
    "\ts_waitcnt lgkmcnt(1)\n" + 20 * VALU +
    "\ts_waitcnt lgkmcnt(0)\n"
    "\tds_read_b64 v[8:9], v0\n"
    "\tds_read2_b32 v[10:11], v0 offset1:1\n" + 12 * VALU +
    "\tds_write_b32 v0, v1\n"
    "\ts_waitcnt lgkmcnt(1)\n"
    "\t; wave barrier\n"
    "\ts_and_saveexec_b64 s[2:3], vcc\n"
    "\ts_cbranch_execz .LBB0_3\n"
    # a masked block: its wait retires a store only -> earlier
    "\tds_write_b32 v0, v2\n"
    "\ts_waitcnt lgkmcnt(0)\n"
    ".LBB0_3:\n"
    "\ts_or_b64 exec, exec, s[2:3]\n"
    "\t;;#ASMSTART\n\t; STAGE_MARK ST_COM_POS\n\t;;#ASMEND\n"
    # stage C: the load was issued before the branch; the wait stands in the next block -> earlier
    "\tds_read_b32 v12, v0\n"
    "\ts_cbranch_scc1 .LBB0_5\n" + 3 * VALU +
    "\ts_waitcnt vmcnt(0) lgkmcnt(0)\n"
    "\ts_waitcnt vmcnt(0)\n"                        # no lgkmcnt: not an LDS wait
    ".LBB0_5:\n"
    "\t; wave barrier\n"
    "\t;;#ASMSTART\n\t; STAGE_MARK ST_RNE\n\t;;#ASMEND\n"
    "\ts_add_u32 s6, s6, 1\n"
    "\ts_cbranch_scc0 .LBB0_1\n"
    "\tds_read_b32 v13, v0\n"
    "\ts_waitcnt lgkmcnt(0)\n"                       # after the loop: not counted
    "\ts_endpgm\n"
    ".Lfunc_end0:\n"
)


def _census(whole=False):
    items = W.ilc.functions(W.annotate(ASM))["_Z6kernelIiEvv"]
    return W.census(items, whole)


def test_blocks_regions_barriers():
    c = _census()
    # body blocks: .LBB0_1 .. s_cbranch_execz | masked stores | .LBB0_3 .. s_cbranch_scc1 | 3 VALU + waits |
    # .LBB0_5 .. the back branch
    assert c["blocks"] == 5
    assert sum(c["block_sizes"].values()) == 5
    assert c["block_sizes"]["25-99"] == 1 and c["block_sizes"]["1-9"] == 4
    assert c["exec_regions"] == 1
    assert c["wave_barriers"] == 2
    assert c["instructions"] == 53 + 2 + 3 + 5 + 2  # the five blocks, the back branch included


def test_wait_bins():
    c = _census()
    assert c["lgkm_waits"] == 7
    assert c["bins"] == {"0-3": 2, "4-11": 1, "12-23": 1, "24+": 1, "earlier": 2}


def test_stage_attribution():
    c = _census()
    assert list(c["stages"]) == ["ST_KINEMATICS", "ST_COM_POS", "ST_RNE"]
    assert c["stages"]["ST_KINEMATICS"] == {"0-3": 2, "4-11": 0, "12-23": 0, "24+": 0, "earlier": 0}
    assert c["stages"]["ST_COM_POS"] == {"0-3": 0, "4-11": 1, "12-23": 1, "24+": 1, "earlier": 1}
    assert c["stages"]["ST_RNE"] == {"0-3": 0, "4-11": 0, "12-23": 0, "24+": 0, "earlier": 1}


def test_whole_kernel_counts_the_code_around_the_loop():
    c = _census(whole=True)
    assert c["lgkm_waits"] == 9
    # the prologue's scalar load shares the counter: its wait retires no ds_read; the epilogue's read is exposed
    assert c["bins"]["earlier"] == 3 and c["bins"]["0-3"] == 3
    assert list(c["stages"])[-1] == "(after last mark)"


def test_command_line_reads_an_assembly_file(tmp_path):
    p = tmp_path / "k.s"
    p.write_text(ASM)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_wait_cover.py"), "--asm", str(p),
                          "--kernel", "kernelI", "--json"], check=True, capture_output=True, text=True).stdout
    assert json.loads(out)["bins"]["0-3"] == 2
    txt = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_wait_cover.py"), "--asm", str(p),
                          "--kernel", "kernelI"], check=True, capture_output=True, text=True).stdout
    assert "5 basic blocks" in txt and "ST_COM_POS" in txt
