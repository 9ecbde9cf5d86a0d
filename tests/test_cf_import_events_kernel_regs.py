"""The kernels that smatrix_cf_import_events adds (kernels/import_events.hpp k_imp_*) are in the library, spill no vector register
and use no scratch memory, and keep the register counts of the build they were written with (no GPU needed: the counts are read from
the gfx950 code object in smatrix.so through tools/kernel_regs.py, as tests/test_cf_explain_kernel_regs.py does).

VGPRs of that build, and the bound: the count rounded up to the granule of 8 registers (512 per SIMD).  None spills a register,
scalar or vector:
    k_imp_scan_reduce    24          a tile of 2048 sessions per workgroup
    k_imp_scan_part      23 -> 24    one workgroup
    k_imp_scan_apply     36 -> 40    eight sessions' slot counts stay in registers between the scan and the stores
    k_imp_emit           20 -> 24    a lane per slot, k_cf_expand's 20: 8 waves per SIMD; 3 KiB of LDS for the compaction
    k_imp_heads           8          a lane per position: DECR's head pass
The call adds kernels of its own and changes none: what tools/kernel_regs.py prints for smx::k_cf_expand and for the kernels of the
incr / decr write path that the call feeds is, number for number, what it printed before the call was written."""
import re

from tests.test_merge_sim_kernel_regs import counts

IMPORT = {
    "smx::k_imp_scan_reduce": 24,
    "smx::k_imp_scan_part": 24,
    "smx::k_imp_scan_apply": 40,
    "smx::k_imp_emit": 24,
    "smx::k_imp_heads": 8,
}

# kernel -> (sgpr, spilled sgpr, vgpr, spilled vgpr, lds, scratch) of the build before this call
UNCHANGED = {
    "smx::k_cf_expand": (20, 0, 20, 0, 0, 0),
    "smx::k_prep": (106, 12, 71, 0, 8544, 0),
    "smx::k_apply_agg<2, 3u, false, false>": (78, 26, 58, 0, 53256, 0),
    "smx::k_apply_agg<2, 1u, false, false>": (78, 26, 58, 0, 53256, 0),
    "smx::k_apply_agg<2, 3u, true, false>": (78, 30, 60, 0, 53256, 0),
    "smx::k_apply_agg<2, 1u, true, false>": (78, 30, 60, 0, 53256, 0),
    "smx::k_apply_agg_clu<2>": (78, 57, 64, 2, 53320, 12),
    "smx::k_apply_agg<3, 3u, false, false>": (78, 26, 58, 0, 53256, 0),
    "smx::k_apply_agg<3, 1u, false, false>": (78, 26, 58, 0, 53256, 0),
    "smx::k_apply_agg<3, 3u, true, false>": (78, 30, 60, 0, 53256, 0),
    "smx::k_apply_agg<3, 1u, true, false>": (78, 30, 60, 0, 53256, 0),
    "smx::k_apply_agg_clu<3>": (78, 57, 64, 2, 53320, 12),
    "smx::k_apply<2, true>": (78, 44, 87, 0, 264, 0),
    "smx::k_apply<2, false>": (78, 37, 66, 0, 264, 0),
    "smx::k_apply<3, true>": (78, 44, 88, 0, 264, 0),
    "smx::k_apply<3, false>": (78, 37, 67, 0, 264, 0),
    "smx::k_apply_short<2>": (78, 51, 61, 0, 264, 0),
    "smx::k_apply_short<3>": (78, 51, 62, 0, 264, 0),
    "smx::k_apply_wpo<2>": (78, 53, 92, 0, 264, 0),
    "smx::k_apply_wpo<3>": (78, 53, 93, 0, 264, 0),
    "smx::k_apply_wpo_far<2>": (106, 35, 96, 29, 264, 56),
    "smx::k_apply_wpo_far<3>": (106, 35, 96, 32, 264, 68),
    "smx::k_fix_rows<2, 8u>": (106, 10, 74, 0, 22544, 0),
    "smx::k_fix_rows<2, 9u>": (106, 7, 76, 0, 43024, 0),
    "smx::k_fix_rows<3, 8u>": (106, 10, 74, 0, 22544, 0),
    "smx::k_fix_rows<3, 9u>": (106, 7, 76, 0, 43024, 0),
    "smx::k_fix_create": (106, 2, 140, 0, 32808, 0),
    "smx::k_fix_count": (78, 0, 89, 0, 32784, 0),
    "smx::k_fix_scatter": (101, 0, 60, 0, 8, 0),
    "smx::k_grow_plan": (58, 0, 32, 0, 384, 0),
    "smx::k_grow_move": (33, 0, 22, 0, 0, 0),
    "smx::k_grow_finish": (68, 0, 56, 0, 0, 0),
    "smx::k_grow_commit": (54, 0, 86, 0, 224, 0),
    "smx::k_grow_lds<64, 8u, false>": (51, 0, 18, 0, 8, 0),
    "smx::k_grow_lds<256, 11u, false>": (53, 0, 18, 0, 8, 0),
    "smx::k_grow_lds<1024, 13u, false>": (55, 0, 21, 0, 8, 0),
    "smx::k_grow_map<false>": (26, 0, 12, 0, 0, 0),
    "smx::k_rebal": (67, 0, 62, 0, 0, 0),
}


def test_the_import_kernels_are_present_spill_nothing_and_keep_their_registers():
    seen, out = counts("k_imp_")
    for name, max_v in IMPORT.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, s_spilled, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert s_spilled == 0 and v_spilled == 0 and scratch == 0, "%s: %d + %d spilled registers, %d bytes of scratch" % (name, s_spilled, v_spilled, scratch)


def test_the_old_expansion_and_the_write_path_kernels_print_the_lines_they_printed():
    _, out = counts("smx::k_")
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?(\S.*?)\s+sgpr\s+(\d+) \(spilled\s+(\d+)\)\s+vgpr\s+(\d+) \(spilled (\d+)\)\s+lds (\d+)\s+scratch (\d+)", line)
        if m:
            seen[m.group(1).strip()] = tuple(int(g) for g in m.groups()[1:])
    assert len(seen) > 50, "tools/kernel_regs.py found no kernels:\n" + out[:500]
    for name, want in UNCHANGED.items():
        assert name in seen, name
        assert seen[name] == want, "%s: (sgpr, spilled, vgpr, spilled, lds, scratch) = %r, it was %r" % (name, seen[name], want)
