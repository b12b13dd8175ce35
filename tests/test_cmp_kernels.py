"""scripts/cmp_kernels.py on synthetic disassembly text (CPU only, no compiler):
what it calls the same code, the two address-only differences it allows and
counts, and what it must still report."""
import importlib.util
import io
import os

from conftest import ROOT

_spec = importlib.util.spec_from_file_location("cmp_kernels", os.path.join(ROOT, "scripts", "cmp_kernels.py"))
ck = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(ck)

# llvm-objdump -d --no-show-raw-insn, as the tool reads it: a pc read whose
# pair gets a 32-bit literal added, an s_add_u32 that follows no pc read, and
# the assembler's padding behind the last instruction
KERNEL = """
0000000000001a00 <_ZN4rtgo6kernelENS_7KParamsE>:
\ts_load_dwordx2 s[8:9], s[0:1], 0x10                        // 000000001A00: C0060200 00000010
\ts_getpc_b64 s[4:5]                                         // 000000001A08: BE841C00
\ts_add_u32 s4, s4, 0x3f4d8                                  // 000000001A0C: 8004FF04 0003F4D8
\ts_addc_u32 s5, s5, 0                                       // 000000001A14: 8205FF05 00000000
\tv_mov_b32_e32 v1, s8                                       // 000000001A1C: 7E020208
\ts_add_u32 s10, s10, 0x3f4d8                                // 000000001A20: 800AFF0A 0003F4D8
\tglobal_atomic_add_x2 v19, v[18:19], s[4:5]                 // 000000001A28: DD888000 00041213
\ts_endpgm                                                   // 000000001A30: BF810000
\ts_nop 0                                                    // 000000001A34: BF800000
\ts_nop 0                                                    // 000000001A38: BF800000
"""
OTHER = """
0000000000002000 <_ZN4rtgo5otherEv>:
\ts_endpgm                                                   // 000000002000: BF810000
"""


def run(parents, news):
    """-> (failures, the tool's last line, everything it printed)"""
    out = io.StringIO()
    bad = ck.compare_sets([ck.parse(t) for t in parents], [ck.parse(t) for t in news], out=out)
    return bad, out.getvalue().strip().splitlines()[-1], out.getvalue()


def test_parse_drops_addresses_and_keeps_instructions():
    f = ck.parse(KERNEL.replace("1A", "7B").replace("1a00", "7b00"))
    assert list(f) == ["_ZN4rtgo6kernelENS_7KParamsE"]
    assert f == ck.parse(KERNEL)
    assert f["_ZN4rtgo6kernelENS_7KParamsE"][1:3] == ["s_getpc_b64 s[4:5]", "s_add_u32 s4, s4, 0x3f4d8"]


def test_trailing_padding_is_the_same_code():
    more = KERNEL + "\ts_nop 0                                 // 000000001A3C: BF800000\n\t...\n"
    none = KERNEL.replace("\ts_nop 0                                                    // 000000001A34: BF800000\n", "").replace(
        "\ts_nop 0                                                    // 000000001A38: BF800000\n", "")
    assert "s_nop" not in none
    for new in (more, none):
        bad, last, _ = run([KERNEL], [new])
        assert bad == 0
        assert last.startswith("identical: 1, different: 0")
        assert "0 pc-relative literals, 1 functions' trailing padding" in last


def test_literal_after_a_pc_read_is_allowed_and_counted():
    new = KERNEL.replace("s_add_u32 s4, s4, 0x3f4d8", "s_add_u32 s4, s4, 0x1234").replace(
        "s_addc_u32 s5, s5, 0 ", "s_addc_u32 s5, s5, -1 ")
    assert new != KERNEL
    bad, last, text = run([KERNEL], [new])
    assert bad == 0
    assert "allowed: 2 pc-relative literals, 0 functions' trailing padding" in last
    assert "pc-relative literals: _ZN4rtgo6kernelENS_7KParamsE - 2" in text


def test_the_same_literal_without_a_pc_read_differs():
    new = KERNEL.replace("s_add_u32 s10, s10, 0x3f4d8", "s_add_u32 s10, s10, 0x1234")
    assert new != KERNEL
    bad, last, text = run([KERNEL], [new])
    assert bad == 1
    assert "DIFFERS: _ZN4rtgo6kernelENS_7KParamsE - 1 of 8 lines" in text
    assert last.startswith("identical: 0, different: 1")


def test_pc_read_of_another_pair_does_not_excuse_the_literal():
    old = KERNEL.replace("s_getpc_b64 s[4:5]", "s_getpc_b64 s[6:7]")
    new = old.replace("s_add_u32 s4, s4, 0x3f4d8", "s_add_u32 s4, s4, 0x1234")
    assert run([old], [new])[0] == 1


def test_one_register_swapped_differs():
    new = KERNEL.replace("v_mov_b32_e32 v1, s8", "v_mov_b32_e32 v2, s8")
    assert run([KERNEL], [new])[0] == 1
    # also in the pc-relative pair itself: only the literal is free
    new = KERNEL.replace("s_add_u32 s4, s4, 0x3f4d8", "s_add_u32 s4, s6, 0x3f4d8")
    assert run([KERNEL], [new])[0] == 1


def test_one_instruction_missing_in_the_middle_differs():
    new = KERNEL.replace("\tv_mov_b32_e32 v1, s8                                       // 000000001A1C: 7E020208\n", "")
    assert new != KERNEL
    bad, last, _ = run([KERNEL], [new])
    assert bad == 1
    assert last.startswith("identical: 0, different: 1")


def test_kernels_match_by_name_over_the_union_of_each_side():
    bad, last, _ = run([KERNEL + OTHER], [OTHER, KERNEL])
    assert bad == 0
    assert last.startswith("identical: 2, different: 0, only in new: []")


def test_a_kernel_twice_in_the_new_set_fails():
    bad, last, text = run([KERNEL + OTHER], [KERNEL + OTHER, OTHER])
    assert bad == 1
    assert "TWICE in new: _ZN4rtgo5otherEv" in text
    assert last.startswith("identical: 1, different: 1")


def test_a_kernel_missing_from_the_new_set_fails():
    bad, _, text = run([KERNEL + OTHER], [KERNEL])
    assert bad == 1
    assert "MISSING in new: _ZN4rtgo5otherEv" in text
