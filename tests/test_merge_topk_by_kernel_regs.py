"""The kernels of smatrix_merge_topk_by's cosine rank (kernels/merge.hpp: k_mgc_*) are in the library, spill nothing, use no scratch
memory and keep the register counts of the build they were written with (no GPU needed: the counts are read from the gfx950 code
object in smatrix.so, in the manner of tests/test_merge_kernel_regs.py, whose check() this uses).

Each of them carries, beside what its k_mgt_* counterpart holds, a 96-bit rank key per cell, the IEEE double sqrt and division of the
score and the probe of its neighbour's get(y, 0), so none fits k_getrow's 56.  The granule is 8 registers of 512 per SIMD:
    k_mgc_select            78 -> 80: 6 waves per SIMD (a row of at most 128 cells also keeps its two keys in registers)
    k_mgc_emit              64:       8 waves per SIMD, the most a CDNA SIMD holds
    k_mgc_select_big       100 -> 104: 4 waves per SIMD, one 1024-lane workgroup per CU (the launch needs <= 128)
    k_mgc_emit_big<true>    32, <false> 46 -> 48: two 1024-lane workgroups per CU, as the k_mgt_emit_big kernels"""
from tests.test_merge_kernel_regs import check

COSINE = {
    "smx::k_mgc_select": 80,
    "smx::k_mgc_emit": 64,
    "smx::k_mgc_select_big": 104,
    "smx::k_mgc_emit_big<true>": 32,
    "smx::k_mgc_emit_big<false>": 48,
}
LANES_1024 = ("smx::k_mgc_select_big", "smx::k_mgc_emit_big<true>", "smx::k_mgc_emit_big<false>")


def test_cosine_kernels_are_present_keep_their_registers_and_use_no_scratch():
    assert all(COSINE[k] <= 128 for k in LANES_1024)                      # a 1024-lane workgroup cannot launch with more
    check(COSINE, "k_mgc_")
