"""tools/kernel_diff.py reads each kernel's resource metadata from its own block.  In hipcc's amdhsa.kernels list the keys of an item are
in alphabetical order, so .vgpr_count and .vgpr_spill_count FOLLOW .symbol: a reader that closes the block at .symbol books them to the
next kernel and never compares the last kernel's."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
kernel_diff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(kernel_diff)


def _asm(vgpr_a, vgpr_b):
    item = """  - .agpr_count:     0
    .args:
      - .address_space:  global
        .offset:         0
        .size:           8
        .value_kind:     global_buffer
    .group_segment_fixed_size: %d
    .name:           %s
    .private_segment_fixed_size: 0
    .sgpr_count:     20
    .sgpr_spill_count: 0
    .symbol:         %s.kd
    .vgpr_count:     %d
    .vgpr_spill_count: 0
    .wavefront_size: 64
"""
    code = "%s:\n\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n\tv_mov_b32_e32 v0, 0\n\ts_endpgm\n.Lfunc_end%d:\n"
    return (code % ("kern_a", 0) + code % ("kern_b", 1) + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + item % (1024, "kern_a", "kern_a", vgpr_a)
            + item % (2048, "kern_b", "kern_b", vgpr_b) + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n\t.end_amdgpu_metadata\n")


def test_metadata_is_booked_to_its_own_kernel(tmp_path):
    p = tmp_path / "a.s"
    p.write_text(_asm(40, 90))
    ops, meta = kernel_diff.parse(str(p))
    assert meta["kern_a"][".vgpr_count"] == 40 and meta["kern_b"][".vgpr_count"] == 90
    assert meta["kern_a"][".group_segment_fixed_size"] == 1024 and meta["kern_b"][".group_segment_fixed_size"] == 2048
    assert ops["kern_a"] == {"s_load_dwordx2": 1, "v_mov_b32_e32": 1, "s_endpgm": 1}


def test_a_changed_register_count_of_the_last_kernel_is_reported(tmp_path, capsys):
    a, b, c = tmp_path / "a.s", tmp_path / "b.s", tmp_path / "c.s"
    a.write_text(_asm(40, 90))
    b.write_text(_asm(40, 999))
    c.write_text(_asm(40, 90))
    assert kernel_diff.main(str(a), str(c)) == 0
    capsys.readouterr()
    assert kernel_diff.main(str(a), str(b)) == 1
    out = capsys.readouterr().out
    assert "kern_b" in out and ".vgpr_count 90 -> 999" in out and "kern_a: 3 -> 3 instructions (+0.00 %), same counts per opcode, metadata equal" in out
