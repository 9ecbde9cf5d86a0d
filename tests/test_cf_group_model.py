"""CPU, no library call: the group maps of tests/cf_group_helpers.py produce the hard cases of smatrix_cf_recommend_grouped, shown with
the model alone (cf_sim_helpers.SessionModel.ranking and the closed form of the contract) over the world's known contents.  The GPU
test (tests/test_gpu_cf_recommend_grouped.py) compares the library with the same model on the same maps."""
import numpy as np

from tests import cf_group_helpers as G
from tests import cf_sim_helpers as H

COS = (H.SIM_COSINE, 0.0)


def run(name, sess, **kw):
    c = G.case(name)
    i = H.all_sessions().index(sess)
    excl = () if c["exclude"] is None else c["exclude"][i]
    return c, G.grouped(G.cpu_model(), sess, c["k"], *COS, c["group_of"], c["cap"], excl=excl, deny=c["deny"] or (), **kw)


def groups_of(c, ids):
    arr = G.as_array(c["group_of"])
    return [G.group_of_id(arr, b) for b in ids]


def test_the_closed_form_is_the_walk():
    """the model counts ALL candidates of the own group that precede; the contract's walk counts the ones taken: the same result"""
    m = G.cpu_model()
    for c in G.cases():
        arr = G.as_array(c["group_of"])
        for sess in (G.LDS_SESSION, [H.HOT], G.TIE_SESSION, [303, 303, 305, 0, H.NO_HEAD_ITEM]):
            r = m.ranking(sess, *COS)
            taken, used = [], {}
            for i, (b, _) in enumerate(r):
                g = G.group_of_id(arr, b)
                if g == G.GROUP_NONE or used.get(g, 0) < c["cap"]:
                    taken.append(i)
                    used[g] = used.get(g, 0) + 1
            assert G.survivors(r, arr, c["cap"]).tolist() == [i for i in taken], (c["name"], sess)


def test_a_the_lds_session_needs_candidates_beyond_its_best_64():
    m = G.cpu_model()
    assert len(m.ranking(G.LDS_SESSION, *COS)) == 217 and G.LDS_SESSION in H.lds_sessions()
    c, (ids, _, at) = run("a", G.LDS_SESSION)
    assert len(ids) == 10 and sum(i < 64 for i in at) < 10 and max(at) >= 64
    assert at == [0, 1, 2, 64, 80, 100, 120, 140, 160, 180]                # three rounds of 64 candidates still alive


def test_b_the_global_session_reaches_the_end_of_its_ranking():
    r = G.cpu_model().ranking([H.HOT], *COS)
    assert len(r) > 4900 and [H.HOT] in H.global_sessions()
    c, (ids, _, at) = run("b", [H.HOT])
    assert len(ids) == 10 and at[0] == 0 and min(at[1:]) > 4000            # beyond every 4096-slot segment's 64 best
    g = groups_of(c, ids)
    assert g[0] == 7 and G.GROUP_NONE in g[1:] and len(set(g[1:]) - {G.GROUP_NONE}) >= 4


def test_c_among_tied_candidates_the_ascending_id_decides():
    r = G.cpu_model().ranking(G.TIE_SESSION, *COS)
    tied = [(b, s) for b, s in r if b in set(H.TIE_COLUMNS.tolist())]
    assert len(tied) == 40 and len(set(s for _, s in tied)) == 1
    c, (ids, _, _) = run("c", G.TIE_SESSION)
    got = [b for b in ids if b in set(H.TIE_COLUMNS.tolist())]
    assert got == [80000, 80001, 80002, 80003, 80004, 80005]               # three of each group, the lowest ids


def test_d_one_group_for_everybody_gives_cap_results():
    for sess in (G.LDS_SESSION, [H.HOT]):
        c, (ids, _, at) = run("d", sess)
        assert c["cap"] == 2 < c["k"] and at == [0, 1]


def test_e_an_excluded_and_a_denied_id_use_no_quota():
    r = [b for b, _ in G.cpu_model().ranking(G.LDS_SESSION, *COS)]
    c, (ids, _, _) = run("e", G.LDS_SESSION)
    assert r[0] not in ids and r[1] not in ids and r[5] in ids and r[6] in ids and r[9] not in ids and r[11] not in ids
    plain = G.grouped(G.cpu_model(), G.LDS_SESSION, 10, *COS, c["group_of"], 1)[0]
    assert r[0] in plain and r[1] in plain and r[5] not in plain and r[6] not in plain


def test_f_ungrouped_ids_are_never_capped():
    c, (ids, _, _) = run("f", G.LDS_SESSION)
    g = groups_of(c, ids)
    beyond = [b for b in ids if b >= c["group_of"].size]
    marked = [b for b in ids if b < c["group_of"].size and c["group_of"][b] == G.GROUP_NONE]
    assert len(ids) == 10 and len(beyond) > c["cap"] and len(marked) > c["cap"] and g.count(1) == 1 and g.count(2) <= 1
    plain = [b for b, _ in G.cpu_model().ranking(G.LDS_SESSION, *COS)[:10]]
    assert sum(50325 <= b < 50350 for b in plain) > 1                      # the quota of group 1 binds


def test_g_sixty_four_groups_in_one_result():
    for sess in (G.LDS_SESSION, [H.HOT]):
        c, (ids, _, at) = run("g", sess)
        assert c["k"] == 64 and len(ids) == 64 and len(set(groups_of(c, ids))) == 64 and max(at) >= 64


def test_h_the_group_ids_0_and_0xfffffffe():
    c, (ids, _, _) = run("h", G.LDS_SESSION)
    assert sorted(groups_of(c, ids)) == [0, 0, 0xFFFFFFFE, 0xFFFFFFFE]


def test_the_dict_and_the_array_form_of_a_map_agree():
    from libsmatrix_amd.matrix import GROUP_NONE, _group_map
    assert GROUP_NONE == G.GROUP_NONE
    for c in G.cases():
        got = _group_map(c["group_of"])
        assert got.dtype == np.uint32 and got.tobytes() == G.as_array(c["group_of"]).tobytes(), c["name"]
    assert _group_map(None) is None and _group_map({}) is None and _group_map([]) is None
