"""scripts/kernel_isa_diff.py: the normaliser and the comparison, on three short hand-written assemblies."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import kernel_isa_diff as kid  # noqa: E402


def _function(name, number, body, vgpr=8):
    """One function as the compiler prints it: header, body, kernel descriptor, end label."""
    return """
	.text
	.protected	{n} ; -- Begin function {n}
	.globl	{n}
	.p2align	8
	.type	{n},@function
{n}: ; @{n}
; %bb.0:
{body}
	.section	.rodata,"a",@progbits
	.p2align	6, 0x0
	.amdhsa_kernel {n}
		.amdhsa_group_segment_fixed_size 1024
		.amdhsa_private_segment_fixed_size 0
		.amdhsa_next_free_vgpr {vgpr}
		.amdhsa_next_free_sgpr 16
	.end_amdhsa_kernel
	.text
.Lfunc_end{k}:
	.size	{n}, .Lfunc_end{k}-{n}
                                        ; -- End function
""".format(n=name, k=number, body=body, vgpr=vgpr)


LOOP = """	s_load_dword s2, s[0:1], 0x0
	v_mov_b32_e32 v1, 0
.LBB{k}_1:                                ; =>This Inner Loop Header: Depth=1
	v_add_u32_e32 v1, 1, v1
	v_cmp_gt_u32_e32 vcc, 8, v1
	s_cbranch_vccnz .LBB{k}_1
; %bb.2:
	{last}
	s_endpgm"""

A = "_Z5alphaPf"
B = "_Z4betaPf"


def test_only_labels_differ_is_equal():
    # the same two kernels in the other order: every .LBB label carries another function number, the comments another text
    base = _function(A, 0, LOOP.format(k=0, last="global_store_dword v0, v1, s[2:3]")) + \
        _function(B, 1, LOOP.format(k=1, last="global_store_dword v0, v1, s[2:3]"))
    new = _function(B, 0, LOOP.format(k=0, last="global_store_dword v0, v1, s[2:3] ; a comment")) + \
        _function(A, 1, LOOP.format(k=1, last="global_store_dword v0, v1, s[2:3]").replace("\t.p2align\t8", "\t.p2align\t4"))
    res = kid.compare(kid.parse_asm(base), kid.parse_asm(new))
    assert res["total"] == 2 and res["identical"] == 2
    assert res["differing"] == [] and res["only_base"] == [] and res["only_new"] == [] and res["resources"] == []


def test_one_opcode_differs_is_reported_by_name():
    base = _function(A, 0, LOOP.format(k=0, last="global_store_dword v0, v1, s[2:3]")) + \
        _function(B, 1, LOOP.format(k=1, last="global_store_dword v0, v1, s[2:3]"))
    new = _function(A, 0, LOOP.format(k=0, last="global_store_dword v0, v1, s[2:3]")) + \
        _function(B, 1, LOOP.format(k=1, last="global_store_short v0, v1, s[2:3]"), vgpr=9)
    res = kid.compare(kid.parse_asm(base), kid.parse_asm(new))
    assert res["identical"] == 1 and len(res["differing"]) == 1
    d = res["differing"][0]
    assert d["name"] == B and d["insts"] == (7, 7)
    assert sorted(d["opcodes"]) == [("global_store_dword", 1, 0), ("global_store_short", 0, 1)]
    assert res["resources"] == [{"name": B, "changes": [("vgpr", "8", "9")]}]
    text = kid.render(res, resources=True)
    assert "beta(float*)" in text and "global_store_short 0 -> 1" in text and "vgpr 8 -> 9" in text
    assert "alpha" not in text


def test_kernel_missing_on_one_side_is_reported():
    base = _function(A, 0, LOOP.format(k=0, last="global_store_dword v0, v1, s[2:3]")) + \
        _function(B, 1, LOOP.format(k=1, last="global_store_dword v0, v1, s[2:3]"))
    new = _function(A, 0, LOOP.format(k=0, last="global_store_dword v0, v1, s[2:3]"))
    res = kid.compare(kid.parse_asm(base), kid.parse_asm(new))
    assert res["total"] == 1 and res["identical"] == 1
    assert res["only_base"] == [B] and res["only_new"] == []
    assert "only in BASE: 1\n  beta(float*)" in kid.render(res)
    back = kid.compare(kid.parse_asm(new), kid.parse_asm(base))
    assert back["only_base"] == [] and back["only_new"] == [B]
