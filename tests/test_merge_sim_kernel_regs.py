"""The kernels that smatrix_merge_topk_sim and smatrix_cf_recommend_sim add (kernels/merge.hpp k_mgs_*, kernels/recommend.hpp
k_rec_*_sim) are in the library and keep the register counts of the build they were written with (no GPU needed: the counts are
read from the gfx950 code object in smatrix.so, as tests/test_merge_kernel_regs.py does).

The truncation's four, next to their cosine counterparts (VGPRs; the granule is 8 registers of 512 per SIMD).  None spills a
register, scalar or vector, and none uses scratch memory:
    k_mgs_select            78 -> 80   k_mgc_select          78 -> 80     6 waves per SIMD
    k_mgs_emit              64         k_mgc_emit            64           8 waves per SIMD
    k_mgs_select_big        72         k_mgc_select_big     100 -> 104    a 1024-lane workgroup needs <= 128; 72 lets 7 waves per
                                                                          SIMD stay where the cosine kernel's 104 lets 4 -- the new
                                                                          body takes its key arithmetic from the policy
                                                                          (kernels/rank_key.hpp) where the cosine kernel spells it out
    k_mgs_emit_big<true>    32         k_mgc_emit_big<true>  32           two 1024-lane workgroups per CU
    k_mgs_emit_big<false>   46 -> 48   k_mgc_emit_big<false> 46 -> 48     two 1024-lane workgroups per CU
No new kernel falls into a lower waves-per-SIMD class than its counterpart.  The measure and the shrinkage are three more scalar
registers per kernel; k_mgs_emit_big<false> has them only because its filter does not carry the directory, the arena and the row
list a second time (MgSimArgs).

The recommend call's two, next to the filtered call's instances they share their bodies with:
    k_rec_lds_sim<false> 60, <true> 60          k_rec_lds<false> 60, <true> 60         (512 lanes, 80 KiB of LDS: two workgroups per CU)
    k_rec_gl_scan_sim<false> 53, <true> 57      k_rec_gl_scan<false> 54, <true> 58     8 waves per SIMD
No vector register is spilled and no scratch memory is used.  k_rec_lds spills SCALAR registers into lanes of a vector register in
every instance, the existing ones included (33 and 46 before this file was written); the _sim instances spill 43 and 56.  That is
not asserted on: it costs no memory access, and the existing instances are the yardstick."""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libsmatrix_amd", "lib", "smatrix.so")

# kernel (demangled, as tools/kernel_regs.py prints it) -> max VGPRs
TRUNCATION = {
    "smx::k_mgs_select": 80,
    "smx::k_mgs_emit": 64,
    "smx::k_mgs_select_big": 72,
    "smx::k_mgs_emit_big<true>": 32,
    "smx::k_mgs_emit_big<false>": 48,
}
RECOMMEND = {
    "smx::k_rec_lds_sim<false>": 64,
    "smx::k_rec_lds_sim<true>": 64,
    "smx::k_rec_gl_scan_sim<false>": 56,
    "smx::k_rec_gl_scan_sim<true>": 64,
}
LANES_1024 = ("smx::k_mgs_select_big", "smx::k_mgs_emit_big<true>", "smx::k_mgs_emit_big<false>")


def counts(flt):
    """{kernel: (VGPRs, spilled SGPRs, spilled VGPRs, scratch bytes)}"""
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), LIB, flt], capture_output=True, text=True, timeout=600).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?(\S.*?)\s+sgpr\s+(\d+) \(spilled\s+(\d+)\)\s+vgpr\s+(\d+) \(spilled (\d+)\)\s+lds \d+\s+scratch (\d+)", line)
        if m:
            seen[m.group(1).strip()] = (int(m.group(4)), int(m.group(3)), int(m.group(5)), int(m.group(6)))
    return seen, out


def test_the_truncation_kernels_are_present_spill_nothing_and_keep_their_registers():
    assert all(TRUNCATION[k] <= 128 for k in LANES_1024)                  # a 1024-lane workgroup cannot launch with more
    seen, out = counts("k_mgs_")
    for name, max_v in TRUNCATION.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, s_spilled, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert s_spilled == 0 and v_spilled == 0 and scratch == 0, "%s: %d + %d spilled registers, %d bytes of scratch" % (name, s_spilled, v_spilled, scratch)


def test_the_recommend_instances_are_present_and_keep_their_registers():
    seen, out = counts("k_rec_")
    for name, max_v in RECOMMEND.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, _, v_spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert v_spilled == 0 and scratch == 0, "%s: %d spilled vector registers, %d bytes of scratch" % (name, v_spilled, scratch)
    for name in ("smx::k_rec_lds<false>", "smx::k_rec_lds<true>", "smx::k_rec_gl_scan<false>", "smx::k_rec_gl_scan<true>"):
        assert name in seen, name                                         # the existing instances keep their names
