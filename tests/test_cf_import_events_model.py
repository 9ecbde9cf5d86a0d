"""CPU, oracle only: the model of smatrix_cf_import_events (tests/cf_import_events_helpers.py model_ops) is tied to the reference's
example -- with the default arguments its ops leave what examples/cf_recommender.c:36-47 import_preference_set leaves -- and to
hand-checked cases written out as literals."""
from tests.cf_import_events_helpers import FORWARD, NO_SELF, apply_model, cells, model_ops, write_path_sessions


def test_the_defaults_are_the_reference_examples_import(oracle_mod):
    sessions = write_path_sessions()
    assert all(s in sessions for s in ([], [7], [9, 9], [3, 5, 3]))
    ops = model_ops(sessions)
    assert len(ops) == sum(len(s) ** 2 for s in sessions)
    a, b = oracle_mod.Oracle(), oracle_mod.Oracle()
    apply_model(a, ops)
    for s in sessions:
        oracle_mod.cf_import_preference_set(b, s)
    rows = b.list_rows()
    assert sorted(a.list_rows().tolist()) == sorted(rows.tolist())
    for r in rows.tolist():
        ca, cb = cells(a.row_slots(r)), cells(b.row_slots(r))
        assert ca.shape == cb.shape and (ca == cb).all(), r
    assert a.get(9, 9) == b.get(9, 9) >= 2 and a.get(3, 3) == b.get(3, 3) >= 2     # the repeated id counted itself
    a.close(); b.close()


HEADS_1234 = [(1, 0, 1), (2, 0, 1), (3, 0, 1), (4, 0, 1)]


def test_a_window_of_one_is_the_neighbours():
    assert sorted(model_ops([[1, 2, 3, 4]], window=1)) == sorted(
        HEADS_1234 + [(1, 2, 1), (2, 1, 1), (2, 3, 1), (3, 2, 1), (3, 4, 1), (4, 3, 1)])


def test_forward_is_what_came_next():
    assert sorted(model_ops([[1, 2, 3, 4]], window=1, flags=FORWARD)) == sorted(HEADS_1234 + [(1, 2, 1), (2, 3, 1), (3, 4, 1)])
    assert sorted(model_ops([[1, 2, 3, 4]], flags=FORWARD)) == sorted(
        HEADS_1234 + [(1, 2, 1), (1, 3, 1), (1, 4, 1), (2, 3, 1), (2, 4, 1), (3, 4, 1)])


def test_a_repeated_id_counts_against_itself_unless_no_self():
    heads = [(3, 0, 1), (5, 0, 1), (3, 0, 1)]
    assert sorted(model_ops([[3, 5, 3]])) == sorted(heads + [(3, 5, 1), (3, 3, 1), (5, 3, 1), (5, 3, 1), (3, 3, 1), (3, 5, 1)])
    assert sorted(model_ops([[3, 5, 3]], flags=NO_SELF)) == sorted(heads + [(3, 5, 1), (5, 3, 1), (5, 3, 1), (3, 5, 1)])


def test_an_amount_of_zero_keeps_its_place_and_the_pair_amount_is_the_min():
    """positions 0, 1 and 3 count; 0 and 3 are three positions apart although only two of the positions between them count"""
    assert sorted(model_ops([[10, 20, 30, 40]], amounts=[[1, 6, 0, 2]], window=2)) == sorted(
        [(10, 0, 1), (20, 0, 6), (40, 0, 2), (10, 20, 1), (20, 10, 1), (20, 40, 2), (40, 20, 2)])
    assert sorted(model_ops([[10, 20, 30, 40]], amounts=[[1, 6, 0, 2]], window=3)) == sorted(
        [(10, 0, 1), (20, 0, 6), (40, 0, 2), (10, 20, 1), (20, 10, 1), (20, 40, 2), (40, 20, 2), (10, 40, 1), (40, 10, 1)])


def test_two_amounts_of_two_to_the_31_wrap_to_zero(oracle_mod):
    ops = model_ops([[5, 5]], amounts=[[0x80000000, 0x80000000]])
    assert sorted(ops) == sorted([(5, 0, 0x80000000), (5, 0, 0x80000000), (5, 5, 0x80000000), (5, 5, 0x80000000)])
    o = oracle_mod.Oracle()
    apply_model(o, ops[:2])                                            # position 0's head op and pair op
    assert o.get(5, 0) == 0x80000000 and o.get(5, 5) == 0x80000000
    apply_model(o, ops[2:])                                            # position 1's: the same two cells again
    assert o.get(5, 0) == 0 and o.get(5, 5) == 0
    o.close()
