"""The register and LDS budget of every guarded kernel, in one table, and the one loader of what the build has (no GPU needed: the
counts are the metadata notes of the gfx950 code object in smatrix.so, read once per process through tools/kernel_regs.py).
tests/test_kernel_regs.py is the only test that reads this; DESIGN 3.7 says why each bound is what it is.

A BUDGET entry holds:
    vgpr_max          VGPRs; mostly the count of the build the kernel was written with, rounded up to the granule of 8 (512 per SIMD)
    sgpr_spill_max    scalar registers spilled into lanes of a vector register; absent: not asserted (it costs no memory access)
    vgpr_spill_max, scratch_max    default 0
    lds_exact         bytes of LDS, to the byte
    lanes_1024        vgpr_max itself is <= 128: a 1024-lane workgroup, or two of 512 lanes per CU, cannot launch with more
    exact             (sgpr, sgpr_spill, vgpr, vgpr_spill, lds, scratch), number for number; the defaults above do not apply"""
import functools, os, subprocess

from tools.kernel_regs import kernel_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "libsmatrix_amd", "lib", "smatrix.so")
FIELDS = ("sgpr", "sgpr_spill", "vgpr", "vgpr_spill", "lds", "scratch")


@functools.lru_cache(maxsize=None)
def rows():
    """{kernel: {sgpr, sgpr_spill, vgpr, vgpr_spill, lds, scratch}} of the built library; builds it if it is not there, never skips"""
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", os.path.join(ROOT, "libsmatrix_amd", "csrc")], check=True)
    return kernel_table(LIB)


def no_spill(vgpr_max, **more):
    return dict(vgpr_max=vgpr_max, sgpr_spill_max=0, **more)


BUDGET = {
    # kernels/ops.hpp: the frozen op kernels.  exact = what the write path printed before smatrix_cf_import_events was written
    "smx::k_apply_agg<2, 1u, true, false>": dict(vgpr_max=64, exact=(78, 30, 60, 0, 53256, 0)),  # the headline's fold: two 1024-lane workgroups per CU need <= 64
    "smx::k_apply_agg<2, 3u, true, false>": dict(exact=(78, 30, 60, 0, 53256, 0)),
    "smx::k_apply_agg<2, 1u, false, false>": dict(exact=(78, 26, 58, 0, 53256, 0)),
    "smx::k_apply_agg<2, 3u, false, false>": dict(exact=(78, 26, 58, 0, 53256, 0)),
    "smx::k_apply_agg<3, 1u, true, false>": dict(exact=(78, 30, 60, 0, 53256, 0)),
    "smx::k_apply_agg<3, 3u, true, false>": dict(exact=(78, 30, 60, 0, 53256, 0)),
    "smx::k_apply_agg<3, 1u, false, false>": dict(exact=(78, 26, 58, 0, 53256, 0)),
    "smx::k_apply_agg<3, 3u, false, false>": dict(exact=(78, 26, 58, 0, 53256, 0)),
    "smx::k_apply_agg_clu<2>": dict(exact=(78, 57, 64, 2, 53320, 12)),
    "smx::k_apply_agg_clu<3>": dict(exact=(78, 57, 64, 2, 53320, 12)),
    "smx::k_apply<0, false>": dict(vgpr_max=48),                         # GET, lane per op
    "smx::k_apply<2, true>": dict(exact=(78, 44, 87, 0, 264, 0)),
    "smx::k_apply<2, false>": dict(exact=(78, 37, 66, 0, 264, 0)),
    "smx::k_apply<3, true>": dict(exact=(78, 44, 88, 0, 264, 0)),
    "smx::k_apply<3, false>": dict(exact=(78, 37, 67, 0, 264, 0)),
    "smx::k_apply_short<2>": dict(exact=(78, 51, 61, 0, 264, 0)),
    "smx::k_apply_short<3>": dict(exact=(78, 51, 62, 0, 264, 0)),
    "smx::k_apply_wpo<2>": dict(exact=(78, 53, 92, 0, 264, 0)),
    "smx::k_apply_wpo<3>": dict(exact=(78, 53, 93, 0, 264, 0)),
    "smx::k_apply_wpo_far<2>": dict(exact=(106, 35, 96, 29, 264, 56)),
    "smx::k_apply_wpo_far<3>": dict(exact=(106, 35, 96, 32, 264, 68)),
    "smx::k_get_clu": dict(vgpr_max=64),                                 # clustered GET: 8 waves per SIMD

    # kernels/prep_bulk.hpp
    "smx::k_prep": dict(exact=(106, 12, 71, 0, 8544, 0)),
    "smx::k_fix_rows<2, 8u>": dict(exact=(106, 10, 74, 0, 22544, 0)),
    "smx::k_fix_rows<2, 9u>": dict(exact=(106, 7, 76, 0, 43024, 0)),
    "smx::k_fix_rows<3, 8u>": dict(exact=(106, 10, 74, 0, 22544, 0)),
    "smx::k_fix_rows<3, 9u>": dict(exact=(106, 7, 76, 0, 43024, 0)),
    "smx::k_fix_create": dict(exact=(106, 2, 140, 0, 32808, 0)),
    "smx::k_fix_count": dict(exact=(78, 0, 89, 0, 32784, 0)),
    "smx::k_fix_scatter": dict(exact=(101, 0, 60, 0, 8, 0)),

    # kernels/growth.hpp: the scrambled stream's growth round (round 5: k_grow_lds 18 / 18 / 21, k_grow_map 18)
    "smx::k_grow_lds<64, 8u, false>": dict(vgpr_max=24, exact=(51, 0, 18, 0, 8, 0)),
    "smx::k_grow_lds<256, 11u, false>": dict(vgpr_max=24, exact=(53, 0, 18, 0, 8, 0)),
    "smx::k_grow_lds<1024, 13u, false>": dict(vgpr_max=28, exact=(55, 0, 21, 0, 8, 0)),
    "smx::k_grow_map<false>": dict(vgpr_max=20, exact=(26, 0, 12, 0, 0, 0)),
    "smx::k_grow_move": dict(vgpr_max=28, exact=(33, 0, 22, 0, 0, 0)),
    "smx::k_grow_plan": dict(exact=(58, 0, 32, 0, 384, 0)),
    "smx::k_grow_finish": dict(exact=(68, 0, 56, 0, 0, 0)),
    "smx::k_grow_commit": dict(exact=(54, 0, 86, 0, 224, 0)),
    "smx::k_rebal": dict(exact=(67, 0, 62, 0, 0, 0)),

    # kernels/rows.hpp
    "smx::k_getrow<2, true, 0>": dict(vgpr_max=56),                      # the config-3 scan: 8 waves per SIMD, the most a CDNA SIMD holds
    "smx::k_cf_expand": dict(exact=(20, 0, 20, 0, 0, 0)),

    # kernels/merge.hpp: wave-per-row kernels take k_getrow's 56, the 1024-lane segment kernels 64 (two workgroups per CU)
    "smx::k_mg_emit": no_spill(56),
    "smx::k_mg_emit_big<true>": no_spill(64),
    "smx::k_mg_emit_big<false>": no_spill(64),
    "smx::k_mg_emit_csr": no_spill(56),
    "smx::k_mgx_count": no_spill(56),
    "smx::k_mgx_emit": no_spill(56),
    "smx::k_mgx_count_big": no_spill(64),
    "smx::k_mgx_emit_big": no_spill(64),
    "smx::k_mgt_select": no_spill(56),
    "smx::k_mgt_emit": no_spill(56),
    "smx::k_mgt_select_big": no_spill(64),
    "smx::k_mgt_emit_big<true>": no_spill(64),
    "smx::k_mgt_emit_big<false>": no_spill(64),
    "smx::k_mgc_select": no_spill(80),                                   # 78: 6 waves per SIMD; a 96-bit key, sqrt and division do not fit 56
    "smx::k_mgc_emit": no_spill(64),                                     # 64: 8 waves per SIMD
    "smx::k_mgc_select_big": no_spill(104, lanes_1024=True),             # 100: 4 waves per SIMD, one 1024-lane workgroup per CU
    "smx::k_mgc_emit_big<true>": no_spill(32, lanes_1024=True),          # 32: two 1024-lane workgroups per CU, as k_mgt_emit_big
    "smx::k_mgc_emit_big<false>": no_spill(48, lanes_1024=True),         # 46
    "smx::k_mgs_select": no_spill(80),                                   # 78, as k_mgc_select
    "smx::k_mgs_emit": no_spill(64),                                     # 64, as k_mgc_emit
    "smx::k_mgs_select_big": no_spill(72, lanes_1024=True),              # 72: 7 waves per SIMD where k_mgc_select_big's 104 lets 4
    "smx::k_mgs_emit_big<true>": no_spill(32, lanes_1024=True),          # 32
    "smx::k_mgs_emit_big<false>": no_spill(48, lanes_1024=True),         # 46

    # kernels/recommend.hpp: the LDS instances are 512 lanes and the table's 80 KiB, two workgroups per CU; what they spill is scalar
    "smx::k_rec_lds_sim<false>": dict(vgpr_max=64),                      # 60, k_rec_lds<false>'s; spills 43 scalars (k_rec_lds: 33)
    "smx::k_rec_lds_sim<true>": dict(vgpr_max=64),                       # 60; spills 56 (k_rec_lds<true>: 46)
    "smx::k_rec_gl_scan_sim<false>": dict(vgpr_max=56),                  # 53 (k_rec_gl_scan<false>: 54): 8 waves per SIMD
    "smx::k_rec_gl_scan_sim<true>": dict(vgpr_max=64),                   # 57 (k_rec_gl_scan<true>: 58)
    "smx::k_rec_fill": no_spill(64),                                     # 61: a wave per session, 8 waves per SIMD
    "smx::k_rec_fill_grouped": no_spill(56),                             # 56: rec_fill_walk<false>; on its own it was 55
    "smx::k_rec_gl_grouped": no_spill(80, lanes_1024=True),              # 77: the grouped ending alone spills nothing at all
    "smx::k_rec_lds_grouped<false>": no_spill(64, lanes_1024=True),      # 60
    "smx::k_rec_lds_grouped<true>": dict(vgpr_max=64, sgpr_spill_max=10, lanes_1024=True),       # 63
    "smx::k_rec_lds_grouped_sim<false>": dict(vgpr_max=64, sgpr_spill_max=5, lanes_1024=True),   # 61
    "smx::k_rec_lds_grouped_sim<true>": dict(vgpr_max=64, sgpr_spill_max=22, lanes_1024=True),   # 63
    "smx::k_rec_gl_deep": no_spill(72, lanes_1024=True),                 # 70: the deep ending alone spills nothing at all; 7 waves per SIMD
    "smx::k_rec_lds_deep<false>": dict(vgpr_max=72, sgpr_spill_max=8, lanes_1024=True),          # 68
    "smx::k_rec_lds_deep<true>": dict(vgpr_max=72, sgpr_spill_max=19, lanes_1024=True),          # 70
    "smx::k_rec_lds_deep_sim<false>": dict(vgpr_max=72, sgpr_spill_max=15, lanes_1024=True),     # 68
    "smx::k_rec_lds_deep_sim<true>": dict(vgpr_max=72, sgpr_spill_max=37, lanes_1024=True),      # 70
    "smx::k_rec_lds_scoped": dict(vgpr_max=64, sgpr_spill_max=77, lds_exact=4096 * 20, lanes_1024=True),          # 62; the table, and no word beside it
    "smx::k_rec_lds_grouped_scoped": dict(vgpr_max=64, sgpr_spill_max=46, lds_exact=4096 * 20, lanes_1024=True),  # 64
    "smx::k_rec_gl_scan_scoped": no_spill(64, lanes_1024=True),          # 63: the 8-waves-per-SIMD class of k_rec_gl_scan_sim<true>
    "smx::k_rec_fill_scoped": dict(vgpr_max=64, sgpr_spill_max=8, lanes_1024=True),              # 61: rec_fill_walk<true>; on its own it was 60
    "smx::k_rec_scope_bound": no_spill(16, lanes_1024=True),             # 10

    # kernels/import_events.hpp
    "smx::k_imp_scan_reduce": no_spill(24),                              # 24: a tile of 2048 sessions per workgroup
    "smx::k_imp_scan_part": no_spill(24),                                # 23: one workgroup
    "smx::k_imp_scan_apply": no_spill(40),                               # 36: eight sessions' slot counts stay in registers
    "smx::k_imp_emit": no_spill(24),                                     # 20, k_cf_expand's: a lane per slot, 8 waves per SIMD
    "smx::k_imp_heads": no_spill(8),                                     # 8: a lane per position, DECR's head pass

    # kernels/explain.hpp
    "smx::k_exp_prep_items": dict(vgpr_max=48),                          # 45: a wave per session, 8 waves per SIMD; spills 4 scalars
    "smx::k_exp_prep_targets": dict(vgpr_max=24),                        # 22: a lane per target
    "smx::k_exp_terms": dict(vgpr_max=32),                               # 26: a lane per output entry

    # kernels/popular.hpp, kernels/trending.hpp
    "smx::k_pop_keys": no_spill(24),                                     # 17: a lane per directory slot, one head-cell gather
    "smx::k_pop_sort": no_spill(16, lanes_1024=True),                    # 11: one 1024-lane workgroup, 32 KiB of LDS
    "smx::k_trend_keys": no_spill(40),                                   # 33: k_pop_keys' gather, a look-up in base, a 64-bit divide
    "smx::k_trend_sort": no_spill(24, lanes_1024=True),                  # 23: one 1024-lane workgroup, 48 KiB of LDS

    # kernels/select.hpp: the dense radix select; RkValue bounds are those of the hand-written 64-bit select it replaced
    "smx::k_sel_start<smx::RkValue>": no_spill(8),                       # 2: one lane (hand-written: 4)
    "smx::k_sel_hist<smx::RkValue>": no_spill(16),                       # 16: streaming, a 1 KiB LDS histogram, 8 waves per SIMD
    "smx::k_sel_pick<smx::RkValue>": no_spill(16),                       # 12: one wave
    "smx::k_sel_collect<smx::RkValue>": no_spill(24),                    # 22: a ballot per wave, one atomic per workgroup
    "smx::k_sel_start<smx::RkCosine>": no_spill(8),                      # 5
    "smx::k_sel_hist<smx::RkCosine>": no_spill(24),                      # 18: three word planes
    "smx::k_sel_pick<smx::RkCosine>": no_spill(16),                      # 12
    "smx::k_sel_collect<smx::RkCosine>": no_spill(24),                   # 24
}

# (kernel, field, other kernel): the kernel's field is no more than the other's in the same build
NO_MORE_THAN = [
    # the deep and the grouped LDS instances are k_rec_lds's fill body with another ending: they spill no more scalars than it does
    ("smx::k_rec_lds_deep<false>", "sgpr_spill", "smx::k_rec_lds<false>"),
    ("smx::k_rec_lds_deep<true>", "sgpr_spill", "smx::k_rec_lds<true>"),
    ("smx::k_rec_lds_deep_sim<false>", "sgpr_spill", "smx::k_rec_lds_sim<false>"),
    ("smx::k_rec_lds_deep_sim<true>", "sgpr_spill", "smx::k_rec_lds_sim<true>"),
    ("smx::k_rec_lds_grouped<false>", "sgpr_spill", "smx::k_rec_lds<false>"),
    ("smx::k_rec_lds_grouped<true>", "sgpr_spill", "smx::k_rec_lds<true>"),
    ("smx::k_rec_lds_grouped_sim<false>", "sgpr_spill", "smx::k_rec_lds_sim<false>"),
    ("smx::k_rec_lds_grouped_sim<true>", "sgpr_spill", "smx::k_rec_lds_sim<true>"),
    # a scoped kernel takes no more LDS than the kernel it stands beside
    ("smx::k_rec_lds_scoped", "lds", "smx::k_rec_lds_sim<true>"),
    ("smx::k_rec_lds_grouped_scoped", "lds", "smx::k_rec_lds_grouped_sim<true>"),
    ("smx::k_rec_gl_scan_scoped", "lds", "smx::k_rec_gl_scan_sim<true>"),
    ("smx::k_rec_fill_scoped", "lds", "smx::k_rec_fill_grouped"),
]

# only required to be in the library under these names: the yardsticks of the instances above
PRESENT = ["smx::k_rec_lds<false>", "smx::k_rec_lds<true>", "smx::k_rec_gl_scan<false>", "smx::k_rec_gl_scan<true>",
           "smx::k_rec_bound<false>", "smx::k_rec_bound<true>"]

# name part -> the kernels whose names hold it, these and no other: the select has a 96-bit and a 64-bit key
EXACT_FAMILIES = {"smx::k_sel_": {"smx::k_sel_%s<smx::%s>" % (k, p) for k in ("start", "hist", "pick", "collect") for p in ("RkCosine", "RkValue")}}

