"""CPU: the slot-order model of tests/cf_neighbors_helpers.py against the oracle's restatement of examples/cf_recommender.c:50-86
(ora_cf_neighbors), on the guards matrix built one scalar op per call -- ids, order and the scores' bits, for every item and for caps
around the row's length.  And the guards matrix itself: every branch of the score it exists for is really in it, so that no case of
tests/test_gpu_cf_neighbors.py is empty."""
import ctypes as C

import numpy as np
import pytest

from tests import cf_neighbors_helpers as N


@pytest.fixture(scope="module")
def guards(oracle_mod):
    o = N.build_scalar(oracle_mod.Oracle())
    yield o, N.oracle_model(o)
    o.close()


def caps_of(entries):
    return sorted({0, 1, max(entries - 1, 0), entries, entries + 1})


def test_neighbours_are_the_oracles_for_every_item_and_cap(guards, oracle_mod):
    o, model = guards
    seen = 0
    for a in N.GUARD_ITEMS:
        entries = model.entries(a)
        assert entries == oracle_mod.cf_neighbors(o, a, 1 << 20)[0].size
        for cap in caps_of(entries):
            wi, ws = oracle_mod.cf_neighbors(o, a, cap)
            gi, gs = model.neighbours(a, cap)
            assert gi.tolist() == wi.tolist(), (a, cap)
            assert N.bits(gs).tolist() == N.bits(ws).tolist(), (a, cap)
            seen += gi.size
    assert seen > 200 and max(model.entries(a) for a in N.GUARD_ITEMS) == 11          # A: ten pairs and its head


def test_topk_is_the_oracles_list_sorted_by_score_then_slot(guards, oracle_mod):
    o, model = guards
    for a in N.GUARD_ITEMS:
        wi, ws = oracle_mod.cf_neighbors(o, a, 1 << 20)
        order = sorted(range(wi.size), key=lambda i: (-ws[i], i))         # scores are >= 0: ordered like their bits
        for k in (1, 2, 64):
            gi, gs = model.topk(a, k)
            assert gi.tolist() == wi[order[:k]].tolist() and N.bits(gs).tolist() == N.bits(ws[order[:k]]).tolist(), (a, k)


def test_the_guards_matrix_holds_every_case_it_exists_for(guards):
    o, model = guards
    f = N.guard_facts(model)
    for name, pairs in f.items():
        assert pairs, name
    assert (N.A, N.D) in f["val>den"] and (N.B, N.A) in f["val>den"]
    assert {(N.A, N.C), (N.B, N.C), (N.FF, N.A), (0, 0)} <= set(f["val==den"])
    assert {(N.D, N.F), (N.D, N.G)} <= set(f["two_step"])                 # totals 2 and 2, 2 and 8: den 2.0000000000000004, 4.000000000000001
    assert {(N.A, N.NOROW), (N.A, N.Z), (N.A, N.NOHEAD), (N.HI1, N.NOROW)} <= set(f["tb==0"])
    assert {a for a, _ in f["ta==0"]} == {N.NOHEAD, N.Z}
    assert f["dead"] == [(N.A, N.DEADC)]
    assert {(N.A, N.A), (N.FF, N.FF), (N.HI, N.HI), (0, 0)} <= set(f["self"])
    assert len(f["ff_item"]) == 6 and {a for a, _ in f["ff_neighbour"]} >= {0, N.A, N.NOHEAD, N.HI, N.TOP, N.FF}
    assert (N.TOP, N.FF) in f["val_ff"] and (N.HI, N.TOP) in f["val_ff"] and (N.HI, N.TOP) in f["total_ff"]
    # sqrt(2^32 - 1) squared rounds back to 2^32 - 1: a value of 2^32 - 1 over two such totals is num == den, score 1.0
    assert (N.HI, N.TOP) in f["val==den"]
    # the head decremented to 0 is an empty cell: no key-0 entry, and row 0's own (0, 49) entry scores 49 / (7 * 7)
    assert 0 not in model.candidates(N.Z).id.tolist() and model.entries(N.Z) == 3
    assert 0 in model.candidates(N.A).id.tolist() and model.entries(N.ONLY_HEAD) == 1
    assert model.entries(N.NOROW) == 0 and model.entries(N.GUARD_ABSENT) == 0 and o.row_info(N.NOROW) is None
    # get(0, 0) = 49 is the total of every (0, total) entry: A's is 25 / (5 * 7), not 25 / 5 > 1 -> 0
    c = model.candidates(N.A)
    head = c.id.tolist().index(0)
    assert c.tb[head] == 49 and c.score[head] == 25.0 / 35.0 and (N.A, 0) in f["head_entry_scores"]
    # B's head was set after its pairs: its key-0 cell is not the table's first
    assert model.candidates(N.B).slot[model.candidates(N.B).id.tolist().index(0)] > 0


def test_the_model_over_the_compiled_reference_is_the_oracles_list(oracle_mod):
    """the same scalar ops into the real reference: its tables and totals feed the model the oracle's bytes"""
    if not oracle_mod.have_reference():
        pytest.skip("oracle/_ref/libsmatrix_ref.so not built (needs the reference's sources)")
    r, o = N.build_scalar(oracle_mod.Reference()), N.build_scalar(oracle_mod.Oracle())
    model = N.oracle_model(r)
    for a in N.GUARD_ITEMS:
        for cap in caps_of(model.entries(a)):
            wi, ws = oracle_mod.cf_neighbors(o, a, cap)
            gi, gs = model.neighbours(a, cap)
            assert gi.tolist() == wi.tolist() and N.bits(gs).tolist() == N.bits(ws).tolist(), (a, cap)
    r.close(); o.close()


def test_the_examples_own_routine_where_the_reference_build_has_it(oracle_mod):
    if not oracle_mod.have_reference():
        pytest.skip("oracle/_ref/libsmatrix_ref.so not built (needs the reference's sources)")
    lib = C.CDLL(oracle_mod.REF_SO)
    if not hasattr(lib, "cf_cosine"):
        pytest.skip("the reference build does not expose cf_cosine: examples/cf_recommender.c does not compile as shipped (no brace at :50-51, "
                    "undeclared pset and row) and is not part of the library; ora_cf_neighbors restates it")
    lib.cf_cosine.restype = C.c_double
    lib.cf_cosine.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32]
    r = N.build_scalar(oracle_mod.Reference())
    model = N.oracle_model(r)
    for a in N.GUARD_ITEMS:
        c = model.candidates(a)
        got = np.array([lib.cf_cosine(r._h, int(b), int(v), c.ta) for b, v in zip(c.id, c.val)], np.float64)
        assert N.bits(got).tolist() == N.bits(c.score).tolist(), a
    r.close()
