"""GPU (-m gpu): the session calls at the edges of their hash tables (kernels/recommend.hpp: k_rec_bound's tiers and sizes, rec_slot /
rec_find at high load and across the last slot, the global tier's chunk tasks and segments, the endings at 64 / 65).

The cases are tests/cf_table_helpers.py's, built over the matrix's own row sizes; tests/test_cf_table_model.py proves without a GPU,
over the oracle, that each stands where it claims.  Here every case first shows the same from the matrix itself (check_case: the plan,
the exact need, and one free slot more than the table has keys -- a case that cannot show it is not run), then runs

    the top-k call      cf_recommend_filtered, k = 64, plain and with sim="jaccard", shrink=0.5; plain also through the _dev flavour
    cf_rank             the case's targets, or default_targets of its ranking
    cf_recommend_grouped   id % 23, at most 2 of a group: a cap that binds
    cf_recommend_deep   k = 100

with the case's exclusion list and the module's deny list.  Expected: cf_sim_helpers.SessionModel over the matrix's own
export("sorted").  Ids, counts and the scores' BYTES over every entry; the host flavours zero-fill behind a count, the _dev flavour
leaves its caller's words."""
import numpy as np
import pytest

from libsmatrix_amd import SparseMatrix
from tests import cf_fill_helpers as F
from tests import cf_group_helpers as G
from tests import cf_rank_helpers as R
from tests import cf_scope_helpers as S
from tests import cf_sim_helpers as H
from tests import cf_table_helpers as T

pytestmark = pytest.mark.gpu

K, DEEP_K = 64, 100
MEASURES = (("cosine", 0.0), ("jaccard", 0.5))
SENT_ID, SENT_SCORE, SENT_COUNT = 0xABCDEF, -7.5, 99


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


class World:
    pass


@pytest.fixture(scope="module")
def world():
    w = World()
    w.m = SparseMatrix()
    T.build(w.m)
    w.export = w.m.export("sorted")
    for got, want in zip(w.export, H.sorted_export_of(T.world_contents())):
        assert got.tobytes() == want.tobytes()
    w.model = H.SessionModel(w.export)
    for a, slots in T.EXPECTED_SLOTS.items():
        assert w.m.row_info(a)[0] == slots, a
    w.cases = T.all_cases(w.m, w.model)
    w.groups, w.scopes = T.group_map(), T.scope_map()
    w.rankings, w.alone = {}, {}
    yield w
    w.m.close()


def ranking(w, c, sim, shrink):
    key = (c.name, sim, shrink)
    if key not in w.rankings:
        w.rankings[key] = w.model.ranking(c.sess, H.SIMS[sim], shrink, None, c.excl, T.DENY)
    return w.rankings[key]


def targets_of(w, c):
    return c.targets if c.targets is not None else T.default_targets(c.sess, ranking(w, c, "cosine", 0.0))


def check_rows(tag, got, want, zero_filled=True):
    """got: (ids[n, k], scores[n, k], counts[n]) of a call; want: per session (ids, scores)"""
    ids, sc, cnt = got[:3]
    for s, (wi, ws) in enumerate(want):
        c = int(cnt[s])
        assert c == len(wi), (tag, s, c, len(wi))
        assert ids[s, :c].tolist() == list(wi), (tag, s)
        assert sc[s, :c].tobytes() == np.asarray(ws, np.float64).tobytes(), (tag, s)
        if zero_filled:
            assert not ids[s, c:].any() and not sc[s, c:].any(), (tag, s)
        else:
            assert (ids[s, c:] == SENT_ID).all() and (sc[s, c:] == SENT_SCORE).all(), (tag, s)


def cut(r, k):
    return [b for b, _ in r[:k]], [s for _, s in r[:k]]


def flat(seqs, dtype=np.uint32):
    off = np.zeros(len(seqs) + 1, np.uint64)
    np.cumsum([len(s) for s in seqs], out=off[1:])
    return off, np.ascontiguousarray(np.concatenate([np.asarray(s, dtype) for s in seqs] + [np.zeros(0, dtype)]), dtype=dtype)


def topk_dev(w, sessions, exclude, k):
    """the plain top-k call's _dev flavour into outputs full of sentinels -> (ids[n, k], scores[n, k], counts[n])"""
    import torch
    n = len(sessions)
    off, items = flat(sessions)
    ex_off, ex = flat(exclude)
    bits = np.zeros((max(T.DENY) + 32) // 32, np.uint32)
    for b in T.DENY:
        bits[b >> 5] |= np.uint32(1 << (b & 31))
    dev = torch.device("cuda", torch.cuda.current_device())
    st = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(st):
        up = lambda a, t: torch.from_numpy(np.concatenate([a, np.zeros(1, a.dtype)]).view(t)).to(dev)    # noqa: E731  (never empty)
        d_off, d_items, d_exoff, d_ex, d_bits = up(off, np.int64), up(items, np.int32), up(ex_off, np.int64), up(ex, np.int32), up(bits, np.int32)
        d_ids = torch.full((n * k,), SENT_ID, dtype=torch.int32, device=dev)
        d_sc = torch.full((n * k,), SENT_SCORE, dtype=torch.float64, device=dev)
        d_cnt = torch.full((n,), SENT_COUNT, dtype=torch.int32, device=dev)
        w.m.cf_recommend_sim_dev(n, d_off.data_ptr(), d_items.data_ptr(), None, d_exoff.data_ptr(), d_ex.data_ptr(), d_bits.data_ptr(),
                                 max(T.DENY) + 1, "cosine", 0.0, k, d_ids.data_ptr(), d_sc.data_ptr(), d_cnt.data_ptr(), stream=st)
    st.synchronize()
    return (d_ids.cpu().numpy().view(np.uint32).reshape(n, k), d_sc.cpu().numpy().reshape(n, k), d_cnt.cpu().numpy().view(np.uint32))


def run_calls(w, cases, tag=""):
    """every call of the module's docstring over `cases` as ONE batch, each compared with the model over every entry
    -> per case, the bytes of everything the calls returned for it"""
    for c in cases:
        T.check_case(w.m, w.model, c)                                     # the precondition, from the matrix's own rows and export
    sessions, exclude = [c.sess for c in cases], [c.excl for c in cases]
    n = len(cases)
    out = [[] for _ in cases]

    def keep(got):
        for s in range(n):
            out[s].append(tuple(a[s].tobytes() for a in got))

    for sim, shrink in MEASURES:
        rs = [ranking(w, c, sim, shrink) for c in cases]
        got = w.m.cf_recommend_filtered(sessions, K, exclude=exclude, deny=T.DENY, sim=sim, shrink=shrink)
        check_rows((tag, "top-k", sim), got, [cut(r, K) for r in rs])
        keep(got)
    rs = [ranking(w, c, "cosine", 0.0) for c in cases]
    got = topk_dev(w, sessions, exclude, K)
    check_rows((tag, "top-k _dev"), got, [cut(r, K) for r in rs], zero_filled=False)
    keep(got)
    targets = [targets_of(w, c) for c in cases]
    ranks, scores, ncand = w.m.cf_rank(sessions, targets, exclude=exclude, deny=T.DENY)
    t_off = np.concatenate([[0], np.cumsum([len(t) for t in targets])])
    for s, (t, r) in enumerate(zip(targets, rs)):
        want_r, want_s = R.expected(t, r)
        assert int(ncand[s]) == len(r), (tag, "rank", s, int(ncand[s]), len(r))
        assert ranks[t_off[s]:t_off[s + 1]].tolist() == want_r.tolist(), (tag, "rank", s)
        assert scores[t_off[s]:t_off[s + 1]].tobytes() == want_s.tobytes(), (tag, "rank", s)
        out[s].append((ranks[t_off[s]:t_off[s + 1]].tobytes(), scores[t_off[s]:t_off[s + 1]].tobytes(), ncand[s].tobytes()))
    got = w.m.cf_recommend_grouped(sessions, K, w.groups, T.GROUP_CAP, exclude=exclude, deny=T.DENY)
    want = []
    for r in rs:
        at = G.survivors(r, w.groups, T.GROUP_CAP)[:K]
        want.append(([r[i][0] for i in at], [r[i][1] for i in at]))
    check_rows((tag, "grouped"), got, want)
    keep(got)
    got = w.m.cf_recommend_deep(sessions, DEEP_K, exclude=exclude, deny=T.DENY)
    check_rows((tag, "deep"), got, [cut(r, DEEP_K) for r in rs])
    keep(got)
    return out


def alone(w, c):
    if c.name not in w.alone:
        w.alone[c.name] = run_calls(w, [c], c.name)[0]
    return w.alone[c.name]


# ---- the tier cut and the size steps ----------------------------------------------------------------------------------------------
def test_the_tier_cut(world):
    """need 4095 and 4096 in a 4096-slot LDS table, 4097 in an 8192-slot global one, reached by one exclusion id and by one position"""
    w = world
    a, b, c, d = w.cases["cut"]
    assert [T.plan(w.m, x.sess, len(x.excl)) for x in (a, b, c, d)] == [(T.LDS, 12), (T.LDS, 12), (T.GLOBAL, 13), (T.GLOBAL, 13)]
    assert [T.need_of(w.m, x.sess, len(x.excl)) for x in (a, b, c, d)] == [4095, 4096, 4097, 4097]
    res = [alone(w, x) for x in (a, b, c, d)]
    assert res[0] == res[1] == res[2] == res[3]                           # the added ids are no candidates: not a byte differs
    assert len(ranking(w, a, "cosine", 0.0)) > 200


def test_the_size_steps(world):
    w = world
    steps = w.cases["steps"]
    assert [T.need_of(w.m, x.sess, len(x.excl)) for x in steps] == [64, 65, 2048, 2049, 8192, 8193, 16384, 16385]
    for lo, hi in zip(steps[::2], steps[1::2]):
        assert T.plan(w.m, hi.sess, len(hi.excl))[1] == T.plan(w.m, lo.sess, len(lo.excl))[1] + 1
        assert alone(w, lo) == alone(w, hi), (lo, hi)                      # one exclusion id more: twice the table, the same bytes


# ---- load and wrap ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["lds 4096", "global 8192"])
def test_a_table_full_to_within_the_rows_free_slots(world, which):
    w = world
    c = w.cases["load"][which]
    lg, keys = T.check_case(w.m, w.model, c)
    assert T.need_of(w.m, c.sess, len(c.excl)) == 1 << lg == (4096, 8192)[which] and 1 <= (1 << lg) - keys.size <= 16
    targets, inside, _ = T.load_targets(w.model, c, lg)
    assert len(inside) >= 8
    loaded = T.Case(c.name + ", targets in the longest run", c.sess, c.excl, c.want, c.need, targets)
    run_calls(w, [loaded], loaded.name)


@pytest.mark.parametrize("which", [0, 1], ids=["lds 4096", "global 8192"])
def test_a_probe_chain_across_the_last_slot(world, which):
    w = world
    c = w.cases["wrap"][which]
    lg, keys = T.check_case(w.m, w.model, c)
    assert lg == 12 + which and int((T.home(keys, lg) >= (1 << lg) - 16).sum()) >= 80
    back, front = T.wrap_run(T.occupied(keys, lg))
    assert back >= 16 and front >= 64
    alone(w, c)


def test_fill_and_scope_on_the_tier_cut_and_the_load_cases(world):
    w = world
    cases = w.cases["cut"] + w.cases["load"]
    for c in cases:
        T.check_case(w.m, w.model, c)
        assert T.plan(w.m, c.sess, len(c.excl), scope=T.SCOPE_LIST) == c.want
    sessions, exclude = [c.sess for c in cases], [c.excl for c in cases]
    fill = T.fill_list()
    got = w.m.cf_recommend_filled(sessions, K, fill, exclude=exclude, deny=T.DENY)
    want = [F.filled(w.model, c.sess, K, H.SIM_COSINE, 0.0, fill, None, c.excl, T.DENY) for c in cases]
    check_rows("filled", got, [(i, s) for i, s, _ in want])
    assert got[3].tolist() == [ns for _, _, ns in want]
    assert any(ns < len(i) for i, _, ns in want) and any(ns == K for _, _, ns in want)
    universe = T.universe()
    got = w.m.cf_recommend_scoped(sessions, K, w.scopes, [T.SCOPE_LIST] * len(cases), mode="only", fill=fill, exclude=exclude, deny=T.DENY)
    want = [S.scoped(w.model, c.sess, K, H.SIM_COSINE, 0.0, w.scopes, w.scopes.size, T.SCOPE_LIST, S.ONLY, universe, None, 64, fill, None,
                     c.excl, T.DENY) for c in cases]
    check_rows("scoped", got, [(i, s) for i, s, _ in want])
    assert got[3].tolist() == [ns for _, _, ns in want]
    assert 0 < want[0][2] and any(0 < ns < len(i) for i, _, ns in want)


# ---- exact duplicate detection ------------------------------------------------------------------------------------------------------
def test_a_session_of_8192_and_of_8193_positions_scores_its_hub_once(world):
    w = world
    a, b = w.cases["dedup"]
    assert (len(a.sess), len(b.sess)) == (T.REC_DEDUP_MAX, T.REC_DEDUP_MAX + 1)
    assert T.plan(w.m, a.sess) == (T.GLOBAL, 14) and T.plan(w.m, b.sess) == (T.GLOBAL, 15)       # (the arena holds 3 * 4096 cells and more)
    once = T.Case("the hub once", [T.HUB], (), T.plan(w.m, [T.HUB]))          # (the three rankings are one: so are the default targets)
    assert alone(w, a) == alone(w, b) == alone(w, once)


# ---- the global tier's tasks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", range(4), ids=["16-slot rows", "512 and 1024", "one segment holds all", "a segment below k"])
def test_global_tier_tasks(world, which):
    w = world
    c = w.cases["tasks"][which]
    assert T.plan(w.m, c.sess, len(c.excl)) == (T.GLOBAL, 13)
    if which == 0:
        assert all(w.m.row_info(a)[0] == 16 for a in c.sess)
    if which >= 2:
        r = [b for b, _ in ranking(w, c, "cosine", 0.0)]
        in_seg1 = sum(int(T.home(np.uint32(b), 13)) >= T.REC_SEG for b in r)
        assert in_seg1 == (0, 5)[which - 2] and all(int(T.home(np.uint32(b), 13)) < T.REC_SEG - 512 for b in r[:64])
    alone(w, c)
    if which == 3:                                                        # ... and below a smaller k: segment 1 holds 5
        got = w.m.cf_recommend_filtered([c.sess], 3, exclude=[c.excl], deny=T.DENY)
        check_rows("k 3", got, [cut(ranking(w, c, "cosine", 0.0), 3)])


# ---- the endings ----------------------------------------------------------------------------------------------------------------------
def test_endings_at_64_and_65_ties_with_the_last_id_and_item_0(world):
    w = world
    by = {c.name: c for c in w.cases["endings"]}
    for tier in (T.LDS, T.GLOBAL):
        assert len(ranking(w, by["64 candidates, " + tier], "cosine", 0.0)) == 64
        assert len(ranking(w, by["65 candidates, " + tier], "cosine", 0.0)) == 65
        assert [b for b, _ in ranking(w, by["tie at 63 .. 65, " + tier], "cosine", 0.0)[62:65]] == [T.T1, T.T2, T.M32]
        assert [b for b, _ in ranking(w, by["tie at 62 .. 64, " + tier], "cosine", 0.0)[61:64]] == [T.T1, T.T2, T.M32]
    for c in w.cases["endings"]:
        assert T.plan(w.m, c.sess, len(c.excl)) == c.want
        alone(w, c)
    for name in ("64 candidates, ", "tie at 63 .. 65, ", "[0, a], ", "[a, 0, 0], ", "[0], "):
        assert alone(w, by[name + T.LDS]) == alone(w, by[name + T.GLOBAL]), name       # the tier changes no byte


def test_64_and_65_rank_targets(world):
    w = world
    for c in w.cases["targets"]:
        assert len(c.targets) in (64, 65) and T.plan(w.m, c.sess) == c.want
        alone(w, c)


# ---- everything in one call -----------------------------------------------------------------------------------------------------------
def test_one_batch_of_every_case_in_shuffled_order(world):
    """lds_list and big_list are filled by atomics in any order, and the global sessions share one group's buffer: every session's
    bytes are those of the session called alone"""
    w = world
    cases = [c for cs in w.cases.values() for c in cs]
    big = sum(1 << c.want[1] for c in cases if c.want and c.want[0] == T.GLOBAL)
    assert big < T.REC_GROUP_SLOTS and sum(1 for c in cases if c.want and c.want[0] == T.GLOBAL) >= 15
    order = np.random.default_rng(99).permutation(len(cases))
    cases = [cases[i] for i in order]
    mixed = run_calls(w, cases, "mixed")
    for c, got in zip(cases, mixed):
        assert got == alone(w, c), c
