"""The record-emission kernels of smatrix_merge / smatrix_import_csr (kernels/merge.hpp) keep their register budget (no GPU
needed: the counts are read from the gfx950 code object in smatrix.so).

k_mg_emit streams row tables like k_getrow and hides the latency of its loads the same way, by residency: its bound is k_getrow's
(tests/test_kernel_regs.py: 56 VGPRs -> 8 waves per SIMD, the most a CDNA SIMD holds; the granule is 8 registers, 512 per SIMD),
so its occupancy is never lower.  The segment kernels run 1024-lane workgroups: two of them per CU need <= 64.  None of them may
use scratch memory."""
import os, re, subprocess, sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libsmatrix_amd", "lib", "smatrix.so")

# kernel (demangled, as tools/kernel_regs.py prints it) -> max VGPRs
BOUNDS = {
    "smx::k_mg_emit": 56,
    "smx::k_mg_emit_big<true>": 64,
    "smx::k_mg_emit_big<false>": 64,
    "smx::k_mg_emit_csr": 56,
}


def test_emit_kernels_keep_their_registers_and_use_no_scratch():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_regs.py"), LIB, "k_mg_"], capture_output=True, text=True, timeout=600).stdout
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
