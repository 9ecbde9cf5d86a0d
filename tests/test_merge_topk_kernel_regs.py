"""The kernels of smatrix_merge_topk (kernels/merge.hpp, k_mgt_*) keep the register budget of the kernels they stand beside
(no GPU needed: the counts are read from the gfx950 code object in smatrix.so).

The reasons are those of tests/test_merge_kernel_regs.py: the wave-per-row kernels stream row tables like k_getrow and hide the
latency of their loads by residency, so their bound is k_getrow's (56 VGPRs -> 8 waves per SIMD, the most a CDNA SIMD holds);
the 1024-lane kernels run two workgroups per CU with <= 64.  None of them may spill or use scratch memory -- the selection (a
64-bit rank key, a radix pass with ballots and LDS adds, the walk over the 256 bins) has to fit into that, SGPRs included: the
1024-lane selection walks the bins without the shuffle scan's lane tests for that reason."""
import os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libsmatrix_amd", "lib", "smatrix.so")

# kernel (demangled, as tools/kernel_regs.py prints it) -> max VGPRs
BOUNDS = {
    "smx::k_mgt_select": 56,
    "smx::k_mgt_emit": 56,
    "smx::k_mgt_select_big": 64,
    "smx::k_mgt_emit_big<true>": 64,
    "smx::k_mgt_emit_big<false>": 64,
}


def test_topk_merge_kernels_keep_their_registers_and_use_no_scratch():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), LIB, "k_mgt_"], capture_output=True, text=True, timeout=600).stdout
    seen = {}
    for line in out.splitlines():
        m = re.match(r"(?:void )?(\S.*?)\s+sgpr\s+(\d+) \(spilled\s+(\d+)\)\s+vgpr\s+(\d+) \(spilled (\d+)\)\s+lds \d+\s+scratch (\d+)", line)
        if m:
            seen[m.group(1).strip()] = (int(m.group(4)), int(m.group(3)) + int(m.group(5)), int(m.group(6)))
    for name, max_v in BOUNDS.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, spilled, scratch = seen[name]
        assert v <= max_v, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert spilled == 0 and scratch == 0, "%s: %d spilled registers, %d bytes of scratch" % (name, spilled, scratch)
