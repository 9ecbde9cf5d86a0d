"""Every guarded kernel keeps its register budget (no GPU needed: the counts are read from the code object in smatrix.so).  The
budgets are the one table of tests/kernel_budget.py; one test id per kernel, so a failure names the kernel.

Round 6 found out why this has to be a test: code shared with the dense-id mechanisms (rest_enter inlined into grow_lds_task, an
eight-window scan in grow_map_body) took the SCRAMBLED stream's k_grow_lds from 18 to 93-96 registers and k_grow_map from 18 to 48,
and the frozen growth round lost 0.035 ms per step before an A/B against the round-5 tree showed it (profiles/r06_ab_vs_r05.txt).
The headline's bounds are the counts of the build the driver's BENCH figures come from, with a few registers of slack for compiler
noise; DESIGN 3.7 has the rest."""
import pytest

from tests.kernel_budget import BUDGET, EXACT_FAMILIES, FIELDS, NO_MORE_THAN, PRESENT, rows


@pytest.mark.parametrize("name", BUDGET, ids=[n.replace("smx::", "") for n in BUDGET])      # ids without the namespace: no "::" inside a test id
def test_kernel_keeps_its_budget(name):
    entry = BUDGET[name]
    assert name in rows(), "kernel %s is not in the library (renamed? update tests/kernel_budget.py and DESIGN 3.1)" % name
    row = rows()[name]
    if "exact" in entry:
        bounds = {"vgpr": entry.get("vgpr_max")}
        for f, want in zip(FIELDS, entry["exact"]):
            assert row[f] == want, "%s: %s = %d, it was %d" % (name, f, row[f], want)
    else:
        bounds = {"vgpr": entry["vgpr_max"], "sgpr_spill": entry.get("sgpr_spill_max"), "vgpr_spill": entry.get("vgpr_spill_max", 0),
                  "scratch": entry.get("scratch_max", 0)}
        if "lds_exact" in entry:
            assert row["lds"] == entry["lds_exact"], "%s: lds = %d, it has to be %d" % (name, row["lds"], entry["lds_exact"])
    for f, most in bounds.items():
        assert most is None or row[f] <= most, "%s: %s = %d, the bound is %d" % (name, f, row[f], most)
    if entry.get("lanes_1024"):
        assert entry["vgpr_max"] <= 128, "%s: vgpr_max = %d, a 1024-lane workgroup cannot launch with more than 128" % (name, entry["vgpr_max"])


def test_no_more_than_the_kernel_beside_it():
    for name, f, other in NO_MORE_THAN:
        assert rows()[name][f] <= rows()[other][f], "%s: %s = %d, %s has %d" % (name, f, rows()[name][f], other, rows()[other][f])


def test_the_yardstick_kernels_keep_their_names():
    for name in PRESENT:
        assert name in rows(), "kernel %s is not in the library" % name


def test_families_are_instantiated_for_these_keys_and_no_other():
    for part, names in EXACT_FAMILIES.items():
        assert {n for n in rows() if part in n} == names


def test_the_tool_finds_the_kernels():
    assert len(rows()) > 50, "tools/kernel_regs.py found %d kernels" % len(rows())
