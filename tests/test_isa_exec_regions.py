"""tools/isa_exec_regions.py on a small hand-written assembly text (CPU only): the regions of a loop body,
their nesting, retained branches, guards and contents, and the totals."""

import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ASM = """
	.text
_Z4stepv:                               ; @_Z4stepv
	s_load_dwordx2 s[0:1], s[4:5], 0x0
	v_cmp_eq_u32_e64 s[40:41], 0, v0
	s_and_saveexec_b64 s[2:3], s[40:41]     ; outside the loop: not counted
	v_mov_b32_e32 v9, 0
	s_or_b64 exec, exec, s[2:3]
.LBB0_1:                                ; =>This Loop Header: Depth=1
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	v_add_f32_e32 v1, v1, v2
	s_and_saveexec_b64 s[2:3], s[40:41]     ; region 0: hoisted lane mask, branch, two stores
	s_cbranch_execz .LBB0_3
	ds_write_b32 v3, v1
	ds_write_b64 v3, v[4:5] offset:8
.LBB0_3:
	s_or_b64 exec, exec, s[2:3]
	; STAGE_MARK ST_ONE
	v_cmp_gt_f32_e32 vcc, 0, v1
	s_and_saveexec_b64 s[2:3], vcc          ; region 1: data test, branch, an if / else inside
	s_cbranch_execz .LBB0_7
	ds_read_b32 v6, v3
	v_cmp_lt_i32_e64 s[6:7], 3, v0
	s_and_saveexec_b64 s[4:5], s[6:7]       ; region 2 (depth 1): then side
	s_xor_b64 s[4:5], exec, s[4:5]
	s_cbranch_execz .LBB0_5
	v_mul_f32_e32 v1, v1, v6
	v_mul_f32_e32 v1, v1, v6
.LBB0_5:
	s_andn2_saveexec_b64 s[4:5], s[4:5]     ; region 3 (depth 1): else side, joins to the outer save
	s_cbranch_execz .LBB0_7
	global_load_dword v7, v[8:9], off
	v_mov_b32_e32 v1, 0
.LBB0_7:
	s_or_b64 exec, exec, s[2:3]
	v_readlane_b32 s8, v40, 3
	v_readlane_b32 s9, v40, 4
	s_and_saveexec_b64 s[2:3], s[8:9]       ; region 4: reloaded mask, no branch, VALU only
	v_mov_b32_e32 v2, v1
	s_or_b64 exec, exec, s[2:3]
	; STAGE_MARK ST_TWO
	s_add_i32 s10, s10, -1
	s_cmp_lg_u32 s10, 0
	s_cbranch_scc1 .LBB0_1
	s_endpgm
.Lfunc_end0:
"""


def test_regions_of_hand_written_body():
    ier = _tool("isa_exec_regions")
    items = ier.ilc.functions(ier.iwc.annotate(ASM))["_Z4stepv"]
    regs, tot = ier.regions(items)
    assert [r["depth"] for r in regs] == [0, 0, 1, 1, 0]
    assert [r["branch"] for r in regs] == [True, True, True, True, False]
    assert [r["guard"] for r in regs] == ["mask", "cmp", "cmp", "mask", "mask-spill"]
    assert [r["stage"] for r in regs] == ["ST_ONE", "ST_TWO", "ST_TWO", "ST_TWO", "ST_TWO"]
    r0, r1, r2, r3, r4 = regs
    assert (r0["size"], r0["lds_write"], r0["lds_read"], r0["valu"], r0["store_only"]) == (3, 2, 0, 0, True)
    # the outer region holds everything up to the join, the nested regions' instructions included
    assert (r1["size"], r1["lds_read"], r1["valu"], r1["vmem"], r1["store_only"]) == (12, 1, 4, 1, False)
    assert (r2["size"], r2["valu"]) == (4, 2)  # s_xor, branch, two multiplies
    assert (r3["size"], r3["vmem"], r3["valu"]) == (3, 1, 1)
    assert (r4["size"], r4["valu"], r4["lds_write"]) == (1, 1, 0)
    assert tot["regions"] == 5 and tot["top_level"] == 3
    assert tot["branches_retained"] == 4 and tot["s_cbranch_execz"] == 4
    assert tot["saveexec"] == 5 and tot["top_mask_store_only"] == 1 and tot["lane_rw"] == 2
    assert tot["top_small_branch_mask"] == 1  # region 0; region 4 keeps no branch, region 1 is a data test
    text = ier.report("_Z4stepv", regs, tot)
    assert "ST_ONE" in text and "regions 5" in text


def test_whole_kernel_counts_the_region_outside_the_loop():
    ier = _tool("isa_exec_regions")
    items = ier.ilc.functions(ier.iwc.annotate(ASM))["_Z4stepv"]
    regs, tot = ier.regions(items, whole=True)
    assert tot["regions"] == 6 and regs[0]["guard"] == "cmp" and not regs[0]["branch"]
