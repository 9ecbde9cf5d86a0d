"""GPU (-m gpu): which kernel instances a session call runs, for every selection the host makes (libsmatrix_amd/csrc/
smx_recommend.inc): ending (top-k, rank, grouped, deep) x filter (nothing given, something given) x score (the cosine, a measure) x
flavour (host, _dev).  The selection is made at run time, and a wrong row of it is a wrong kernel instance whose output can look
plausible: every case is compared with the model, byte for byte.

Every call takes TWO sessions, one per tier -- cf_deep_helpers.LDS_SESSION and GLOBAL_SESSIONS[0] --, so every case launches both
tiers' kernels of its selection.  Expected results: cf_sim_helpers.SessionModel over the matrix's own export("sorted"), through
cf_rank_helpers.expected_all, cf_group_helpers.grouped and cf_fill_helpers.filled.  Ids, counts and ranks must be equal, the scores'
uint64 bit patterns too, and the unused entries: zeros from the host flavour, what they held before from _dev."""
import numpy as np
import pytest

from tests import cf_deep_helpers as D
from tests import cf_fill_helpers as F
from tests import cf_group_helpers as G
from tests import cf_rank_helpers as R
from tests import cf_sim_helpers as H
from tests.test_gpu_cf_deep import JUNK_ID, JUNK_SCORE, on_device
from tests.test_gpu_cf_rank import DENY, build_world, rank_dev
from tests.test_gpu_cf_recommend_fill import fill_dev
from tests.test_gpu_cf_recommend_grouped import grouped_dev
from tests.test_gpu_cf_sim import LDS_SLOTS, World, need, same_bytes

pytestmark = pytest.mark.gpu

SESSIONS = [list(D.LDS_SESSION), list(D.GLOBAL_SESSIONS[0])]
MEASURES = [("cosine", 0.0), ("jaccard", 0.5)]
WEIGHTS = [[0.5, 2.0, 1.25, 3.0], [1.5]]
K, DEEP_K = 10, 65
GROUPS = G.case("a")                                                      # k = 10, cap = 1: the quota binds in both sessions


@pytest.fixture(scope="module", autouse=True)
def device():
    import libsmatrix_amd
    assert libsmatrix_amd.device_available(), "no HIP device: the product has no CPU fallback"


@pytest.fixture(scope="module")
def world():
    w = World()
    w.m = build_world()
    w.export = w.m.export("sorted")
    for got, want in zip(w.export, H.sorted_export_of(H.world_contents())):
        assert got.tobytes() == want.tobytes()                            # the matrix holds what the model test looked at
    w.model = H.SessionModel(w.export)
    assert need(w.m, SESSIONS[0]) <= LDS_SLOTS < need(w.m, SESSIONS[1])   # one session per tier
    assert need(w.m, SESSIONS[0], 4) <= LDS_SLOTS                         # ... with its exclusion list as well
    w.filters = {}
    yield w
    w.m.close()


def filters(w, given, sim, shrink):
    """-> dict(weights, exclude, deny) as the calls take them: None each with nothing given; otherwise weights, per session the
    places 0 and 2 of its unfiltered ranking and the ids 0 and 305, and test_gpu_cf_rank's deny list"""
    if not given:
        return dict(weights=None, exclude=None, deny=None)
    if (sim, shrink) not in w.filters:
        rankings = [w.model.ranking(s, H.SIMS[sim], shrink) for s in SESSIONS]
        w.filters[sim, shrink] = dict(weights=WEIGHTS, exclude=[[r[0][0], r[2][0], 0, 305] for r in rankings], deny=DENY)
    return w.filters[sim, shrink]


def rankings(w, sim, shrink, f):
    return [w.model.ranking(s, H.SIMS[sim], shrink, None if f["weights"] is None else f["weights"][i],
                            () if f["exclude"] is None else f["exclude"][i], f["deny"] or ()) for i, s in enumerate(SESSIONS)]


def check(got, want, k, zero_filled, tag):
    """(ids[n,k], scores[n,k], counts[n]) against want, per session (ids as a list, scores float64)"""
    ids, sc, cnt = got
    assert ids.dtype == np.uint32 and sc.dtype == np.float64 and cnt.dtype == np.uint32 and ids.shape == sc.shape == (len(want), k)
    for s, (wi, ws) in enumerate(want):
        c = len(wi)
        assert int(cnt[s]) == c, (tag, s, int(cnt[s]), c)
        assert ids[s, :c].tolist() == wi, (tag, s)
        assert sc[s, :c].view(np.uint64).tolist() == np.asarray(ws, np.float64).view(np.uint64).tolist(), (tag, s)
        if zero_filled:
            assert not ids[s, c:].any() and sc[s, c:].tobytes() == bytes(8 * (k - c)), (tag, s)
        else:                                                             # _dev leaves what it does not own
            assert (ids[s, c:] == JUNK_ID).all() and (sc[s, c:] == JUNK_SCORE).all(), (tag, s)


@pytest.mark.parametrize("flavour", ["host", "dev"])
@pytest.mark.parametrize("sim,shrink", MEASURES)
@pytest.mark.parametrize("given", [False, True], ids=["plain", "filtered"])
@pytest.mark.parametrize("ending", ["topk", "rank", "grouped", "deep"])
def test_every_selection_is_the_models_bytes(world, ending, given, sim, shrink, flavour):
    w, host = world, flavour == "host"
    f = filters(w, given, sim, shrink)
    measure = dict(sim=sim, shrink=shrink)
    tag = (ending, given, sim, flavour)
    full = rankings(w, sim, shrink, f)
    if ending == "rank":
        targets = [R.target_list(s, r) for s, r in zip(SESSIONS, rankings(w, sim, shrink, filters(w, False, sim, shrink)))]
        want = R.expected_all(w.model, SESSIONS, targets, sim, shrink, f["weights"], f["exclude"], f["deny"] or ())
        got = w.m.cf_rank(SESSIONS, targets, **f, **measure) if host else rank_dev(w.m, SESSIONS, targets, sim, shrink, **f)
        assert got[0].dtype == np.uint32 and got[1].dtype == np.float64 and got[2].dtype == np.uint32
        assert got[2].tolist() == want[2].tolist() and got[0].tolist() == want[0].tolist(), tag
        assert got[1].view(np.uint64).tolist() == want[1].view(np.uint64).tolist(), tag
        assert ((want[0] >= 64) & (want[0] != R.RANK_NONE)).any() and (want[0] == R.RANK_NONE).any()
        return
    if ending == "topk":
        k = K
        want = [([b for b, _ in r[:k]], [v for _, v in r[:k]]) for r in full]
        got = w.m.cf_recommend_filtered(SESSIONS, k, **f, **measure) if host else on_device(w.m, "cf_recommend_sim_dev", SESSIONS, k, sim, shrink, **f)
    elif ending == "grouped":
        k, c = GROUPS["k"], GROUPS["cap"]
        assert G.as_array(GROUPS["group_of"]).size and c < k
        want = [G.grouped(w.model, s, k, H.SIMS[sim], shrink, GROUPS["group_of"], c, None if f["weights"] is None else f["weights"][i],
                          () if f["exclude"] is None else f["exclude"][i], f["deny"] or ())[:2] for i, s in enumerate(SESSIONS)]
        assert all(wi != [b for b, _ in r[:k]] for (wi, _), r in zip(want, full))      # the quota changes both results
        got = (w.m.cf_recommend_grouped(SESSIONS, k, GROUPS["group_of"], c, **f, **measure) if host
               else grouped_dev(w.m, SESSIONS, k, GROUPS["group_of"], c, sim, shrink, **f))
    else:
        k = DEEP_K
        want = [([b for b, _ in r[:k]], [v for _, v in r[:k]]) for r in full]
        assert all(len(wi) == k for wi, _ in want)                        # both sessions use the 65th place
        got = w.m.cf_recommend_deep(SESSIONS, k, **f, **measure) if host else on_device(w.m, "cf_recommend_deep_dev", SESSIONS, k, sim, shrink, **f)
    check(got, want, k, host, tag)


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_a_grouped_call_that_cannot_bind_and_a_deep_call_up_to_64_are_the_sim_call(world, sim, shrink):
    w = world
    measure = dict(sim=sim, shrink=shrink)
    plain, d_plain = w.m.cf_recommend_filtered(SESSIONS, K, **measure), on_device(w.m, "cf_recommend_sim_dev", SESSIONS, K, sim, shrink)
    for group_of, cap in [(None, 1), (GROUPS["group_of"], K), (GROUPS["group_of"], 64)]:
        assert same_bytes(w.m.cf_recommend_grouped(SESSIONS, K, group_of, cap, **measure), plain), cap
        assert same_bytes(grouped_dev(w.m, SESSIONS, K, group_of, cap, sim, shrink), d_plain), cap
    assert same_bytes(w.m.cf_recommend_deep(SESSIONS, 64, **measure), w.m.cf_recommend_filtered(SESSIONS, 64, **measure))
    assert same_bytes(on_device(w.m, "cf_recommend_deep_dev", SESSIONS, 64, sim, shrink), on_device(w.m, "cf_recommend_sim_dev", SESSIONS, 64, sim, shrink))


@pytest.mark.parametrize("sim,shrink", MEASURES)
def test_the_fill_call_behind_a_filtered_top_k(world, sim, shrink):
    """a deny list that leaves the LDS-tier session nothing and the global-tier session three candidates: both are filled"""
    w = world
    f = dict(weights=WEIGHTS, exclude=[[F.FRESH[2], 305], [F.FRESH[3]]], deny=F.heavy_deny())
    fill = F.fill_list()
    want = [F.filled(w.model, s, K, H.SIMS[sim], shrink, fill, f["weights"][i], f["exclude"][i], f["deny"]) for i, s in enumerate(SESSIONS)]
    assert [n for _, _, n in want] == [0, 3] and all(len(wi) == K for wi, _, _ in want)
    for flavour in ("host", "dev"):
        got = w.m.cf_recommend_filled(SESSIONS, K, fill, **f, sim=sim, shrink=shrink) if flavour == "host" else fill_dev(w.m, SESSIONS, K, fill, sim, shrink, **f)
        check(got[:3], [(wi, ws) for wi, ws, _ in want], K, flavour == "host", (flavour, sim))
        assert got[3].dtype == np.uint32 and got[3].tolist() == [n for _, _, n in want], (flavour, sim)
