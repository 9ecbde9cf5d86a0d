"""The kernels that smatrix_cf_explain adds (kernels/explain.hpp k_exp_*) are in the library, spill no vector register and use no
scratch memory, and keep the register counts of the build they were written with (no GPU needed: the counts are read from the gfx950
code object in smatrix.so through tools/kernel_regs.py, as tests/test_merge_sim_kernel_regs.py does).

VGPRs of that build, and the bound: the count rounded up to the granule of 8 registers (512 per SIMD):
    k_exp_prep_items     45 -> 48    a wave per session; 8 waves per SIMD.  Spills 4 SCALAR registers into lanes of a vector register
                                     (no memory access; not asserted on, as for k_rec_lds)
    k_exp_prep_targets   22 -> 24    a lane per target
    k_exp_terms          26 -> 32    a lane per output entry: one get per lane, 8 waves per SIMD
The call adds kernels of its own and changes none: the lines tools/kernel_regs.py prints for smx::k_rec_* and smx::k_mg* are the same
before and after it."""
from tests.test_merge_sim_kernel_regs import counts

EXPLAIN = {
    "smx::k_exp_prep_items": 48,
    "smx::k_exp_prep_targets": 24,
    "smx::k_exp_terms": 32,
}


def test_the_explain_kernels_are_present_spill_no_vector_register_and_keep_their_registers():
    seen, out = counts("k_exp_")
    for name, max_v in EXPLAIN.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, _, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert v_spilled == 0 and scratch == 0, "%s: %d spilled vector registers, %d bytes of scratch" % (name, v_spilled, scratch)
