"""The kernel that smatrix_cf_recommend_grouped_fill adds (kernels/recommend.hpp k_rec_fill_grouped) is in the library, spills no
register, scalar or vector, uses no scratch memory, and keeps the register count of the build it was written with (no GPU needed: the
counts are read from the gfx950 code object in smatrix.so through tools/kernel_regs.py, as tests/test_cf_fill_kernel_regs.py does).

VGPRs of that build, and the bound: the count rounded up to the granule of 8 registers (512 per SIMD):
    k_rec_fill_grouped   56 -> 56    a wave per session; k_rec_fill's loops and one more 64-step shuffle loop for the two counts, the
                                     groups of the result in one more register per lane: 8 waves per SIMD, as k_rec_fill (61 -> 64)
The kernel is rec_fill_walk<false>, the body it shares with k_rec_fill_scoped (written out on its own it was 55).  k_rec_fill stays
written out beside it: tests/test_cf_fill_kernel_regs.py, unchanged, pins k_rec_fill at 64 and no spill, and the other register tests
pin the rest."""
from tests.test_merge_sim_kernel_regs import counts

NEW = {"smx::k_rec_fill_grouped": 56}


def test_the_new_kernel_is_present_spills_nothing_and_keeps_its_registers():
    seen, out = counts("smx::k_rec_fill")
    for name, max_v in NEW.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, s_spilled, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert s_spilled == 0 and v_spilled == 0 and scratch == 0, "%s: %d + %d spilled registers, %d bytes of scratch" % (name, s_spilled, v_spilled, scratch)
    assert "smx::k_rec_fill" in seen                                      # the fill call's kernel keeps its name
