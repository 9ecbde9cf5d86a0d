"""The kernels that smatrix_cf_trending runs (kernels/trending.hpp k_trend_*, kernels/select.hpp k_sel_*<RkCosine>) are in the library, spill no register
and use no scratch memory, and keep the register counts of the build they were written with (no GPU needed: the counts are read from
the gfx950 code object in smatrix.so through tools/kernel_regs.py, as tests/test_cf_fill_kernel_regs.py does).

VGPRs of that build, and the bound: the count rounded up to the granule of 8 registers (512 per SIMD):
    k_trend_keys               33 -> 40    a lane per directory slot: one head-cell gather, one look-up in base's directory, a 64-bit
                                           divide and the score; 112 bytes of LDS for the workgroup's seven words
    k_sel_start<RkCosine>       5 ->  8    one lane
    k_sel_hist<RkCosine>       18 -> 24    streaming, three word planes, a 1 KiB LDS histogram: 8 waves per SIMD
    k_sel_pick<RkCosine>       12 -> 16    one wave
    k_sel_collect<RkCosine>    24          streaming; a ballot per wave, one atomic per workgroup that takes any key
    k_trend_sort               23 -> 24    one 1024-lane workgroup, 48 KiB of LDS, two look-ups per result entry
Next to them the popular call's kernels (k_pop_keys, k_sel_*<RkValue>, k_pop_sort) print 17, 2, 16, 12, 22 and 11: the 96-bit key costs
two to twelve registers and no class of waves per SIMD.  tests/test_cf_fill_kernel_regs.py pins those, and the other *_kernel_regs
files what the other kernels print."""
from tests.test_merge_sim_kernel_regs import counts

NEW = {
    "smx::k_trend_keys": 40,
    "smx::k_sel_start<smx::RkCosine>": 8,
    "smx::k_sel_hist<smx::RkCosine>": 24,
    "smx::k_sel_pick<smx::RkCosine>": 16,
    "smx::k_sel_collect<smx::RkCosine>": 24,
    "smx::k_trend_sort": 24,
}


def test_the_new_kernels_are_present_spill_nothing_and_keep_their_registers():
    seen, out = counts("smx::k_")
    for name, max_v in NEW.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, s_spilled, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert s_spilled == 0 and v_spilled == 0 and scratch == 0, "%s: %d + %d spilled registers, %d bytes of scratch" % (name, s_spilled, v_spilled, scratch)
    assert NEW["smx::k_trend_sort"] <= 128                                # a 1024-lane workgroup cannot launch with more


def test_the_select_is_instantiated_for_the_96_bit_and_the_64_bit_key_and_no_other():
    seen, _ = counts("smx::k_sel_")
    assert sorted(seen) == sorted("smx::k_sel_%s<smx::%s>" % (k, p) for k in ("start", "hist", "pick", "collect") for p in ("RkCosine", "RkValue"))
