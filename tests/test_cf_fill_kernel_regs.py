"""The kernels that smatrix_cf_popular and smatrix_cf_recommend_fill run (kernels/popular.hpp k_pop_keys / k_pop_sort, the dense select
of kernels/select.hpp as its 64-bit instances k_sel_*<RkValue>, kernels/recommend.hpp k_rec_fill) are in the library, spill no
register and use no scratch memory, and keep the register counts of the build they were written with (no GPU needed: the counts are
read from the gfx950 code object in smatrix.so through tools/kernel_regs.py, as tests/test_cf_import_events_kernel_regs.py does).

VGPRs of this build, and the bound: the count of the hand-written 64-bit select that these instances
replaced, rounded up to the granule of 8 registers (512 per SIMD):
    k_pop_keys                17 -> 24    a lane per directory slot, one head-cell gather; 48 bytes of LDS for the workgroup's OR and count
    k_sel_start<RkValue>       2 ->  8    one lane (the hand-written kernel: 4)
    k_sel_hist<RkValue>       16          streaming, keys stored whole, a 1 KiB LDS histogram: 8 waves per SIMD
    k_sel_pick<RkValue>       12 -> 16    one wave
    k_sel_collect<RkValue>    22 -> 24    streaming; a ballot per wave, one atomic per workgroup that takes any key
    k_pop_sort                11 -> 16    one 1024-lane workgroup, 32 KiB of LDS
    k_rec_fill                61 -> 64    a wave per session; the compiler unrolls the 64-step shuffle loops: 8 waves per SIMD all the same
tests/test_cf_trending_kernel_regs.py pins the 96-bit instances and that there are no others; tests/test_cf_import_events_kernel_regs.py,
test_cf_explain_kernel_regs.py and test_merge_sim_kernel_regs.py, unchanged, pin what the other kernels print."""
from tests.test_merge_sim_kernel_regs import counts

NEW = {
    "smx::k_pop_keys": 24,
    "smx::k_sel_start<smx::RkValue>": 8,
    "smx::k_sel_hist<smx::RkValue>": 16,
    "smx::k_sel_pick<smx::RkValue>": 16,
    "smx::k_sel_collect<smx::RkValue>": 24,
    "smx::k_pop_sort": 16,
    "smx::k_rec_fill": 64,
}


def test_the_new_kernels_are_present_spill_nothing_and_keep_their_registers():
    seen, out = counts("smx::k_")
    for name, max_v in NEW.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, s_spilled, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert s_spilled == 0 and v_spilled == 0 and scratch == 0, "%s: %d + %d spilled registers, %d bytes of scratch" % (name, s_spilled, v_spilled, scratch)
    assert NEW["smx::k_pop_sort"] <= 128                                  # a 1024-lane workgroup cannot launch with more
