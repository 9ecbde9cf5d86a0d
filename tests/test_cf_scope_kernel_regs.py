"""The kernels that smatrix_cf_recommend_scoped adds (kernels/recommend.hpp k_rec_lds_scoped, k_rec_lds_grouped_scoped,
k_rec_gl_scan_scoped, k_rec_fill_scoped, k_rec_scope_bound) are in the library, spill no vector register, use no scratch memory, stay
at or below 128 VGPRs and at or below the LDS of the kernels they stand beside, and keep the counts of the build they were written
with (no GPU needed: the counts are read from the gfx950 code object in smatrix.so through tools/kernel_regs.py).

VGPRs of that build and the bound (the count rounded up to the granule of 8 registers, 512 per SIMD), the scalar registers spilled
into lanes of a vector register pinned at that build's count, and the kernel each stands beside:
    k_rec_lds_scoped           62 -> 64   77 spilled   81920 B   k_rec_lds_sim<true>          60, 56 spilled, 81920 B
    k_rec_lds_grouped_scoped   64 -> 64   46 spilled   81920 B   k_rec_lds_grouped_sim<true>  63, 22 spilled, 81920 B
    k_rec_gl_scan_scoped       63 -> 64    0 spilled       0 B   k_rec_gl_scan_sim<true>      57,  0 spilled
    k_rec_fill_scoped          61 -> 64    8 spilled       0 B   k_rec_fill_grouped           56,  0 spilled
    k_rec_scope_bound          10 -> 16    0 spilled       0 B
The two LDS instances keep the table's 80 KiB and not a byte more: two workgroups per CU, as the kernels beside them.  Their scalar
spills are the shared fill body's plus the scope's five words and the loop over the list; a scalar spill costs no memory access.  Every
kernel stays in the 8-waves-per-SIMD class (<= 64 VGPRs) of its neighbour.
k_rec_fill_scoped is rec_fill_walk<true>, the body it shares with k_rec_fill_grouped (written out on its own it was 60); the other
kernels that existed keep their code: the other register tests pin what they print."""
import re

from tests.test_merge_sim_kernel_regs import counts

# kernel -> (max VGPRs, max scalar registers spilled, the kernel it stands beside or None)
NEW = {
    "smx::k_rec_lds_scoped": (64, 77, "smx::k_rec_lds_sim<true>"),
    "smx::k_rec_lds_grouped_scoped": (64, 46, "smx::k_rec_lds_grouped_sim<true>"),
    "smx::k_rec_gl_scan_scoped": (64, 0, "smx::k_rec_gl_scan_sim<true>"),
    "smx::k_rec_fill_scoped": (64, 8, "smx::k_rec_fill_grouped"),
    "smx::k_rec_scope_bound": (16, 0, None),
}


def lds_bytes(out):
    return {m.group(1).strip(): int(m.group(2)) for m in re.finditer(r"(?m)^(?:void )?(\S.*?)\s+sgpr .*? lds (\d+)\s+scratch", out)}


def test_the_new_kernels_are_present_and_keep_their_registers_spills_and_lds():
    seen, out = counts("k_rec_")
    lds = lds_bytes(out)
    for name, (max_v, max_s, beside) in NEW.items():
        assert name in seen, "kernel %s is not in the library:\n%s" % (name, out[:500])
        v, s_spilled, v_spilled, scratch = seen[name]
        assert v <= max_v <= 128, "%s: %d VGPRs, the bound is %d" % (name, v, max_v)
        assert v_spilled == 0 and scratch == 0, "%s: %d spilled vector registers, %d bytes of scratch" % (name, v_spilled, scratch)
        assert s_spilled <= max_s, "%s: %d spilled scalar registers, the bound is %d" % (name, s_spilled, max_s)
        if beside is not None:
            assert beside in seen, beside
            assert lds[name] <= lds[beside], "%s: %d bytes of LDS, %s has %d" % (name, lds[name], beside, lds[beside])
    assert lds["smx::k_rec_lds_scoped"] == lds["smx::k_rec_lds_grouped_scoped"] == 4096 * 20      # the table, and no word beside it


def test_the_kernels_beside_them_keep_their_names():
    seen, _ = counts("k_rec_")
    for name in ("smx::k_rec_fill", "smx::k_rec_fill_grouped", "smx::k_rec_bound<true>", "smx::k_rec_bound<false>", "smx::k_rec_lds_sim<true>",
                 "smx::k_rec_lds_grouped_sim<true>", "smx::k_rec_gl_scan_sim<true>"):
        assert name in seen, name
