"""tools/kernel_diff.py on small hand-written assembly: kernels that moved to
another file and another function index compare equal; a changed instruction,
a changed descriptor, a missing kernel and a kernel defined twice are reported."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import kernel_diff  # noqa: E402


def _kernel(sym, idx, insn="v_mov_b32_e32 v0, 0", vgpr=4):
    return (f"\t.globl\t{sym}\n\t.type\t{sym},@function\n{sym}:            ; @{sym}\n; %bb.0:\n"
            f"\ts_cbranch_scc1 .LBB{idx}_2\n\t{insn}      ; a comment\n.LBB{idx}_2:\n\ts_endpgm\n"
            f"\t.section\t.rodata,\"a\",@progbits\n\t.amdhsa_kernel {sym}\n\t\t.amdhsa_next_free_vgpr {vgpr}\n"
            f"\t.end_amdhsa_kernel\n\t.text\n.Lfunc_end{idx}:\n\t.size\t{sym}, .Lfunc_end{idx}-{sym}\n")


def _write(d, files):
    os.makedirs(d)
    for name, text in files.items():
        with open(os.path.join(d, name), "w") as f:
            f.write(text)
    return str(d)


def test_moved_kernels_match(tmp_path):
    a = _write(tmp_path / "a", {"one.s": _kernel("k_a", 0) + _kernel("k_b", 1)})
    b = _write(tmp_path / "b", {"x.s": _kernel("k_b", 0), "y.s": _kernel("k_a", 7)})
    assert kernel_diff.compare(a, b) == ([], [], [], ["k_a", "k_b"], [])


def test_differences_are_reported(tmp_path):
    a = _write(tmp_path / "a", {"one.s": _kernel("k_a", 0) + _kernel("k_b", 1) + _kernel("k_c", 2) + _kernel("k_d", 3)})
    b = _write(tmp_path / "b", {"x.s": _kernel("k_a", 0, insn="v_mov_b32_e32 v0, 1") + _kernel("k_b", 1, vgpr=8),
                                "y.s": _kernel("k_c", 0) + _kernel("k_e", 1), "z.s": _kernel("k_c", 0)})
    only_a, only_b, differ, same, twice = kernel_diff.compare(a, b)
    assert (only_a, only_b, differ, same, twice) == (["k_d"], ["k_e"], ["k_a", "k_b"], ["k_c"], ["k_c"])
