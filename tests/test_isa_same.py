"""tools/isa_same.py on four tiny synthetic listings (no compiler): a function is the same machine
code when its text from the label to .Lfunc_end, with the block labels' function ordinal masked and
comments stripped, and its .amdhsa_kernel descriptor are the same strings."""
import contextlib
import importlib.util
import io
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_same", os.path.join(ROOT, "tools", "isa_same.py"))
isa_same = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(isa_same)


def _fn(name, ordinal, operand="v1", vgprs=8, note="a comment"):
    return f"""\t.globl\t{name}
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:
\ts_load_dword s0, s[4:5], 0x0          ; {note}
.LBB{ordinal}_1:                        ; =>This Inner Loop Header: Depth=1
\tv_add_u32_e32 v0, v0, {operand}
\ts_cbranch_scc1 .LBB{ordinal}_1
\ts_endpgm
.Lfunc_end{ordinal}:
\t.size\t{name}, .Lfunc_end{ordinal}-{name}
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 6
\t.end_amdhsa_kernel
\t.text
"""


PARENT = _fn("kern_a", 0) + _fn("kern_b", 1) + _fn("kern_c", 2) + _fn("kern_gone", 3)
MOVED = _fn("kern_b", 0, note="another comment") + _fn("kern_a", 1)  # ordinals moved: identical
OPERAND = _fn("kern_c", 0, operand="v2")
DESCRIPTOR = _fn("kern_c", 0, vgprs=9)


def _run(tmp_path, here, *flags):
    """-> (report by function name, exit status) of PARENT against the listings `here`."""
    (tmp_path / "parent.s").write_text(PARENT)
    paths = []
    for i, text in enumerate(here):
        paths.append(str(tmp_path / f"here{i}.s"))
        (tmp_path / f"here{i}.s").write_text(text)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        status = isa_same.main([str(tmp_path / "parent.s"), "--"] + paths + list(flags))
    out = buf.getvalue().splitlines()
    return {ln.split()[-1]: ln for ln in out[:-1]}, status


def test_a_moved_ordinal_is_identical(tmp_path):
    rep, status = _run(tmp_path, [MOVED], "--must-match", "kern_[ab]")
    assert status == 0
    assert rep["kern_a"].startswith("identical") and rep["kern_b"].startswith("identical")


def test_functions_are_matched_across_the_files_of_a_side(tmp_path):
    rep, status = _run(tmp_path, [_fn("kern_a", 0), _fn("kern_b", 0)], "--must-match=kern_[ab]")
    assert status == 0 and rep["kern_a"].startswith("identical") and rep["kern_b"].startswith("identical")


def test_a_changed_operand_differs(tmp_path):
    rep, status = _run(tmp_path, [MOVED, OPERAND])
    assert status == 1
    assert rep["kern_c"].startswith("differs (text;") and "parent 5 lines, here 5" in rep["kern_c"]
    assert rep["kern_a"].startswith("identical")
    # ... and not when only the others have to match
    assert _run(tmp_path, [MOVED, OPERAND], "--must-match", "kern_[ab]")[1] == 0


def test_a_changed_descriptor_field_differs(tmp_path):
    rep, status = _run(tmp_path, [MOVED, DESCRIPTOR])
    assert status == 1 and rep["kern_c"].startswith("differs (descriptor;")


def test_a_missing_function_is_reported_and_fails_under_must_match(tmp_path):
    here = [MOVED + _fn("kern_new", 2)]
    rep, status = _run(tmp_path, here)
    assert rep["kern_gone"].startswith("only in the parent") and rep["kern_c"].startswith("only in the parent")
    assert rep["kern_new"].startswith("only here")
    assert status == 0  # the default: the functions on both sides
    assert _run(tmp_path, here, "--must-match", "kern_gone")[1] == 1
    assert _run(tmp_path, here, "--must-match", "kern_new")[1] == 1
    assert _run(tmp_path, here, "--must-match", "no_such_function")[1] == 1
