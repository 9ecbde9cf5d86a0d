"""CPU: the host model of the export and of getrow_batch (tests/export_helpers.py) against the kernels' own constants, read as
source text, and against the oracle.  The GPU tests that stand on this model are tests/test_gpu_export_edges.py."""
import os
import re

import numpy as np

from tests import export_helpers as H

KERNELS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libsmatrix_amd", "csrc", "kernels")


def constexpr_u32(text, name):
    hit = re.findall(r"constexpr\s+uint32_t\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert len(hit) == 1, (name, hit)
    return int(hit[0])


def test_constants_are_the_kernels():
    for fn, names in H.SOURCE_CONSTANTS.items():
        with open(os.path.join(KERNELS, fn)) as f:
            text = f.read()
        for name, value in names.items():
            assert constexpr_u32(text, name) == value, (fn, name)
    with open(os.path.join(KERNELS, "export.hpp")) as f:
        ex = f.read()
    with open(os.path.join(KERNELS, "rows.hpp")) as f:
        rows = f.read()
    assert re.search(r"constexpr\s+uint32_t\s+EX_TILE\s*=\s*EX_THREADS\s*\*\s*EX_PER_THREAD\s*;", ex)
    assert H.EX_TILE == 4096
    assert "b += EX_THREADS" in ex and H.SCAN_PART_STEP == H.EX_THREADS          # k_ex_scan_part's step
    assert "c <= EX_LDS_SMALL" in ex and "c <= EX_LDS_MID" in ex and "if (c < 2) return;" in ex   # k_ex_classify's tiers
    assert "size > GETROW_WAVE_MAX" in ex and "size > GETROW_WAVE_MAX" in rows
    assert "p0 += 256" in rows and "fetch(w[k], p0 + 128)" in rows and H.WAVE_STEP == 128          # two 128-cell steps in flight
    assert "size >= 2 * GETROW_SEG ? size / GETROW_SEG : 1u" in rows                               # getrow_nseg


def test_table_size_rule():
    assert [H.table_size_for(n) for n in (0, 1, 8, 9, 10, 17, 18, 4097, 4098, 8193, 16385, 16386, 32768)] == \
        [16, 16, 16, 16, 32, 32, 64, 8192, 16384, 16384, 32768, 65536, 65536]


def test_builders():
    x, y, v = H.rows_with_pair_counts([1, 2, 513, 0, 4097], 7, first_row=50)
    assert np.unique(x, return_counts=True)[1].tolist() == [1, 2, 513, 4097] and set(x.tolist()) == {50, 51, 52, 54}
    assert (y != 0).all() and (v != 0).all() and (v == H.pair_value(x, y)).all()
    assert np.unique(x.astype(np.uint64) << np.uint64(32) | y).size == x.size
    assert int(y.max()) > 1 << 31 and int(y.min()) < 1 << 28             # the whole range, not a corner of it
    for b0, b1 in ((0, 1), (1, 2), (2, 3), (3, 0)):
        c = H.columns_varying_in_bytes(4097, b0, b1)
        assert np.unique(c).size == 4097
        for b in range(4):
            n = np.unique((c >> np.uint32(8 * b)) & np.uint32(255)).size
            assert (n > 16) if b in (b0, b1) else (n == 1), (b0, b1, b)
    for n in (1, 2, 4095, 4096, 4097, 40000):
        ids = H.row_list_ids(n, n)
        assert ids.size == n == np.unique(ids).size and H.M32 in ids
        assert n < 2 or 0 in ids
        assert n < 4095 or np.unique(ids[(ids & np.uint32(0xFFFFFF)) == 0xC0FFEE] >> np.uint32(24)).size == 256
    assert H.edge_caps(4096) == [0, 1, 127, 128, 129, 4095, 4096, 4097] and H.edge_caps(8) == [0, 1, 7, 8, 9, 127, 128, 129]


def oracle_export(o):
    """the SORTED export the oracle's contents call for, and every row's slots"""
    xs = np.sort(o.list_rows().astype(np.uint32))
    ptr = np.zeros(xs.size + 1, np.uint64)
    parts, slots = [np.zeros((0, 2), np.uint32)], {}
    for i, x in enumerate(xs.tolist()):
        slots[x] = o.row_slots(x)
        ne = H.nonempty(slots[x])
        parts.append(ne[np.argsort(ne[:, 0], kind="stable")].astype(np.uint32))
        ptr[i + 1] = ptr[i] + np.uint64(ne.shape[0])
    return (xs, ptr, np.concatenate(parts)), slots


def test_model_is_the_oracle(oracle_mod):
    """a few hundred triples on the ids 0 and 0xFFFFFFFF and around them, with the (0, v), (y, 0) and (0, 0) cells of the
    scalar calls: the model of SORTED, of a TABLE walk and of getrow under a cap is what the oracle holds"""
    x, y, v = H.rows_with_pair_counts([1, 2, 3, 9, 10, 17, 40, 0, 130, 65], 11, first_row=0)
    x2, y2, v2 = H.rows_with_pair_counts([5, 33], 12, first_row=H.M32 - 1)
    edge = np.array([[0, H.M32, 5], [H.M32, H.M32, H.M32], [3, 1, 1]], np.uint32)    # the largest column, the all-ones pair
    x, y, v = (np.concatenate(t) for t in ((x, x2, edge[:, 0]), (y, y2, edge[:, 1]), (v, v2, edge[:, 2])))
    keep = np.unique(x.astype(np.uint64) << np.uint64(32) | y, return_index=True)[1]  # (a drawn column may be an edge's)
    x, y, v = x[np.sort(keep)], y[np.sort(keep)], v[np.sort(keep)]
    scalars = [(4, 0, 9), (H.M32, 0, 77), (7, 0, 0), (8, 0, 0), (5, 12345, 0), (7000, 6, 0), (0, 0, 3), (9000, 0, H.M32)]
    assert 7 not in x.tolist() and 8 in x.tolist()                      # Q3 on a new row; (0, 0) on a row that has pairs
    o = oracle_mod.Oracle()
    H.fill(o, x, y, v, scalars)
    want, slots = oracle_export(o)
    got = H.sorted_model(x, y, v, scalars)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.dtype == b.dtype and a.shape == b.shape and (a == b).all(), k
    assert x.size > 300 and {0, 7, H.M32} <= set(got[0].tolist())
    assert {(0, 3), (H.M32, H.M32), (12345, 0), (0, H.M32)} <= set(map(tuple, got[2].tolist()))
    for xx, s in slots.items():
        if xx not in {sc[0] for sc in scalars}:                        # (the y = 0 quirks count `used` their own way)
            assert H.table_size_for(o.rowlen(xx)) == s.shape[0], xx
        full = o.getrow(xx, 8 * (s.shape[0] + 1))
        assert (H.table_row_model(s) == full).all(), xx
        for cap in (1, 2, full.shape[0] - 1, full.shape[0], full.shape[0] + 1):
            if cap >= 1:
                assert (H.table_row_model(s, cap) == o.getrow(xx, 8 * cap)).all(), (xx, cap)
    t = [np.array(list(slots), np.uint32)[::-1]]                        # a TABLE-shaped export in some other row order
    parts = [H.table_row_model(slots[xx]) for xx in t[0].tolist()]
    t += [np.concatenate([[0], np.cumsum([p.shape[0] for p in parts])]).astype(np.uint64), np.concatenate(parts)]
    for a, b in zip(H.table_as_sorted(*t), want):
        assert a.shape == b.shape and (a == b).all()
    offsets, buf, counts = H.getrow_model(slots, [3, 123456, 3], [2, 5, 0], 0xC3C3C3C3, 4)
    assert offsets.tolist() == [0, 2, 7, 7] and counts.tolist() == [2, 0, 0] and buf.size == 22
    assert (buf[:4].reshape(2, 2) == H.table_row_model(slots[3], 2)).all() and (buf[4:] == 0xC3C3C3C3).all()
    o.close()
