"""The kernels that smatrix_cf_recommend_deep adds (kernels/recommend.hpp k_rec_lds_deep<F>, k_rec_lds_deep_sim<F>, k_rec_gl_deep) are in
the library, spill no vector register and use no scratch memory, and keep the register counts of the build they were written with (no
GPU needed: the counts are read from the gfx950 code object in smatrix.so through tools/kernel_regs.py, as
tests/test_cf_grouped_kernel_regs.py does).

VGPRs of that build, and the bound: the count rounded up to the granule of 8 registers (512 per SIMD); and the scalar registers
spilled into lanes of a vector register, pinned at that build's count:
    k_rec_gl_deep                70 -> 72    0 spilled   one 1024-lane workgroup per session, 13.0 KiB of LDS (k_rec_gl_merge: 75)
    k_rec_lds_deep<false>        68 -> 72    8 spilled   512 lanes and 80 KiB of LDS, the table's: two workgroups per CU, as k_rec_lds
    k_rec_lds_deep<true>         70 -> 72   19 spilled
    k_rec_lds_deep_sim<false>    68 -> 72   15 spilled
    k_rec_lds_deep_sim<true>     70 -> 72   37 spilled
k_rec_gl_deep is the deep ending alone (rec_deep_table) and spills nothing, scalar or vector.  The LDS instances are the fill body of
k_rec_lds with that ending behind it; what they spill is the fill body's: the top-k instances of the same bodies spill 33 / 46 / 43 / 56
in the same order (tests/test_merge_sim_kernel_regs.py), and each deep instance stays below its counterpart.  A scalar spill goes into a
lane of a vector register and costs no memory access; the counts are pinned all the same, so that a change which adds to them is seen.
72 registers allow 7 waves per SIMD; two 512-lane workgroups per CU, or one of 1024 lanes, need 4.
The call adds kernels of its own and changes none: tests/test_cf_grouped_kernel_regs.py, test_cf_fill_kernel_regs.py,
test_cf_import_events_kernel_regs.py, test_cf_explain_kernel_regs.py and test_merge_sim_kernel_regs.py, unchanged, pin what the other
kernels print."""
from tests.test_merge_sim_kernel_regs import counts

# kernel -> (max VGPRs, max scalar registers spilled)
NEW = {
    "smx::k_rec_gl_deep": (72, 0),
    "smx::k_rec_lds_deep<false>": (72, 8),
    "smx::k_rec_lds_deep<true>": (72, 19),
    "smx::k_rec_lds_deep_sim<false>": (72, 15),
    "smx::k_rec_lds_deep_sim<true>": (72, 37),
}


def test_the_new_kernels_are_present_and_keep_their_registers_and_spills():
    seen, out = counts("k_rec_")
    for name, (max_v, max_s) in NEW.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, s_spilled, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert v_spilled == 0 and scratch == 0, "%s: %d spilled vector registers, %d bytes of scratch" % (name, v_spilled, scratch)
        assert s_spilled <= max_s, "%s: %d spilled scalar registers, the bound is %d" % (name, s_spilled, max_s)
    assert NEW["smx::k_rec_gl_deep"] == (72, 0)                           # the ending on its own spills nothing at all
    assert all(v <= 128 for v, _ in NEW.values())                         # a 1024-lane workgroup, or two of 512 lanes per CU: 4 waves per SIMD


def test_the_deep_instances_spill_no_more_than_the_fill_body_does_elsewhere():
    """the LDS instances' scalar spills are the shared fill body's: each stays below the top-k instance of the same body"""
    seen, _ = counts("k_rec_")
    for deep, topk in (("smx::k_rec_lds_deep<false>", "smx::k_rec_lds<false>"), ("smx::k_rec_lds_deep<true>", "smx::k_rec_lds<true>"),
                       ("smx::k_rec_lds_deep_sim<false>", "smx::k_rec_lds_sim<false>"), ("smx::k_rec_lds_deep_sim<true>", "smx::k_rec_lds_sim<true>")):
        assert seen[deep][1] <= seen[topk][1], (deep, seen[deep][1], topk, seen[topk][1])
