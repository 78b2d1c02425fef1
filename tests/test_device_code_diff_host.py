"""tools/device_code_diff.py on a few lines of made-up assembly: what it leaves aside and what it must not."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("device_code_diff", os.path.join(ROOT, "tools", "device_code_diff.py"))
dcd = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(dcd)

ASM = """\t.text
\t.type\t{k1},@function
{k1}:
.Lfunc_begin{n}:
\ts_cbranch_scc1 .LBB{n}_2
.Ltmp{t}:                                 ;     Child Loop BB{n}_2 Depth 2
\tv_add_f32 v0, v1, v2
.LBB{n}_2:                                ;   in Loop: Header=BB{n}_1 Depth=1
\ts_endpgm
.Lfunc_end{n}:
\t.amdhsa_kernel {k1}
\t.end_amdhsa_kernel
\t.type\t__hip_cuid_{cuid},@object
\t.type\t{k2},@function
{k2}:
\t{op} v0, v1, v2
\ts_endpgm
\t.amdhsa_kernel {k2}
\t.end_amdhsa_kernel
"""


def _asm(k1="_Z3fooILi4EEvv", k2="_Z3barv", n=0, t=0, cuid="abc", op="v_mul_f32"):
    return ASM.format(k1=k1, k2=k2, n=n, t=t, cuid=cuid, op=op)


def test_functions_are_split_by_name_and_local_label_numbers_do_not_count():
    a, b = dcd.functions(_asm()), dcd.functions(_asm(n=5, t=17, cuid="xyz"))
    assert sorted(a) == ["_Z3barv", "_Z3fooILi4EEvv"]
    assert dcd.differing(a, b) == []


def test_one_changed_instruction_is_one_differing_function():
    assert dcd.differing(dcd.functions(_asm()), dcd.functions(_asm(op="v_add_f32"))) == ["_Z3barv"]
    # a block label is part of the text: only the function index in front of it is not
    assert dcd.differing(dcd.functions(_asm()), dcd.functions(_asm().replace("_2", "_3"))) == ["_Z3fooILi4EEvv"]


def test_rename_map_is_applied_in_one_pass():
    ren = dcd.renamer(["3fooILi=3fooILi0ELi", "8foo_halfILi=3fooILi"])
    assert ren("_Z3fooILi4EEvv _Z8foo_halfILi2ELi4EEvv") == "_Z3fooILi0ELi4EEvv _Z3fooILi2ELi4EEvv"
    old = dcd.functions(ren(_asm()))
    assert dcd.differing(old, dcd.functions(_asm(k1="_Z3fooILi0ELi4EEvv"))) == []
    assert dcd.differing(dcd.functions(_asm()), dcd.functions(_asm(k1="_Z3fooILi0ELi4EEvv"))) == ["_Z3fooILi0ELi4EEvv", "_Z3fooILi4EEvv"]


def test_resource_lines_leave_source_positions_aside():
    rem = ("gat.hip:{ln}:1: remark: Function Name: _Z3barv [-Rpass-analysis=kernel-resource-usage]\n"
           "gat.hip:{ln}:1: remark:     VGPRs: {v} [-Rpass-analysis=kernel-resource-usage]\n")
    a = dcd.resources(rem.format(ln=10, v=12))
    assert a == {"_Z3barv": ["VGPRs: 12"]}
    assert dcd.differing(a, dcd.resources(rem.format(ln=99, v=12))) == []
    assert dcd.differing(a, dcd.resources(rem.format(ln=10, v=13))) == ["_Z3barv"]
