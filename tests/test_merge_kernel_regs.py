"""The kernels of the merge family and of the CSR import (kernels/merge.hpp: k_mg_* of smatrix_merge / smatrix_import_csr, k_mgx_* of
smatrix_merge_scaled, k_mgt_* of smatrix_merge_topk, k_mgc_* of smatrix_merge_topk_by's cosine rank) keep their register budget (no GPU needed: the counts are read from the gfx950
code object in smatrix.so).

The wave-per-row kernels stream row tables like k_getrow and hide the latency of their loads the same way, by residency: their
bound is k_getrow's (tests/test_kernel_regs.py: 56 VGPRs -> 8 waves per SIMD, the most a CDNA SIMD holds; the granule is 8
registers, 512 per SIMD), so their occupancy is never lower.  The segment kernels run 1024-lane workgroups: two of them per CU need
<= 64.  None of them may spill or use scratch memory.  Into that have to fit the scaled merge's transform (a 32 x 32 -> 64 bit
product, an FP64 estimate of the quotient and its correction) and the top-k selection (a 64-bit rank key, a radix pass with ballots
and LDS adds, the walk over the 256 bins), SGPRs included: the 1024-lane selection walks the bins without the shuffle scan's lane
tests for that reason.

The cosine kernels are in the library, spill nothing, use no scratch memory and keep the register counts of the build they were
written with.  Each of them carries, beside what its k_mgt_* counterpart holds, a 96-bit rank key per cell, the IEEE double sqrt and
division of the score and the probe of its neighbour's get(y, 0), so none fits k_getrow's 56.  The granule is 8 registers of 512 per
SIMD:
    k_mgc_select            78 -> 80: 6 waves per SIMD (a row of at most 128 cells also keeps its two keys in registers)
    k_mgc_emit              64:       8 waves per SIMD, the most a CDNA SIMD holds
    k_mgc_select_big       100 -> 104: 4 waves per SIMD, one 1024-lane workgroup per CU (the launch needs <= 128)
    k_mgc_emit_big<true>    32, <false> 46 -> 48: two 1024-lane workgroups per CU, as the k_mgt_emit_big kernels"""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libsmatrix_amd", "lib", "smatrix.so")

# kernel (demangled, as tools/kernel_regs.py prints it) -> max VGPRs
MERGE = {
    "smx::k_mg_emit": 56,
    "smx::k_mg_emit_big<true>": 64,
    "smx::k_mg_emit_big<false>": 64,
    "smx::k_mg_emit_csr": 56,
}
SCALED = {
    "smx::k_mgx_count": 56,
    "smx::k_mgx_emit": 56,
    "smx::k_mgx_count_big": 64,
    "smx::k_mgx_emit_big": 64,
}
TOPK = {
    "smx::k_mgt_select": 56,
    "smx::k_mgt_emit": 56,
    "smx::k_mgt_select_big": 64,
    "smx::k_mgt_emit_big<true>": 64,
    "smx::k_mgt_emit_big<false>": 64,
}
COSINE = {
    "smx::k_mgc_select": 80,
    "smx::k_mgc_emit": 64,
    "smx::k_mgc_select_big": 104,
    "smx::k_mgc_emit_big<true>": 32,
    "smx::k_mgc_emit_big<false>": 48,
}
LANES_1024 = ("smx::k_mgc_select_big", "smx::k_mgc_emit_big<true>", "smx::k_mgc_emit_big<false>")


def check(bounds, flt):
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), LIB, flt], capture_output=True, text=True, timeout=600).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?(\S.*?)\s+sgpr\s+(\d+) \(spilled\s+(\d+)\)\s+vgpr\s+(\d+) \(spilled (\d+)\)\s+lds \d+\s+scratch (\d+)", line)
        if m:
            seen[m.group(1).strip()] = (int(m.group(4)), int(m.group(3)) + int(m.group(5)), int(m.group(6)))
    for name, max_v in bounds.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert spilled == 0 and scratch == 0, "%s: %d spilled registers, %d bytes of scratch" % (name, spilled, scratch)


def test_emit_kernels_keep_their_registers_and_use_no_scratch():
    check(MERGE, "k_mg_")


def test_scaled_merge_kernels_keep_their_registers_and_use_no_scratch():
    check(SCALED, "k_mgx_")


def test_topk_merge_kernels_keep_their_registers_and_use_no_scratch():
    check(TOPK, "k_mgt_")


def test_cosine_kernels_are_present_keep_their_registers_and_use_no_scratch():
    assert all(COSINE[k] <= 128 for k in LANES_1024)                      # a 1024-lane workgroup cannot launch with more
    check(COSINE, "k_mgc_")
