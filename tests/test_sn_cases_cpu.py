"""The inputs of tests/test_gpu_snsolve.py, checked where no device is needed: every case of tests/sn_cases.py is shaped
like a Cholesky factor, is one tree too big for the per-tree kernels, survives the plan builder's worth-it test, stays on
its side of the growth guard, and -- by the model of the schedule in tests/sn_cases.py -- sits exactly on the edge it is
named for.  The table of the edges is checked for completeness at the end."""
import numpy as np
import pytest

import sn_cases as SC

NAMES = [c.name for c in SC.CASES]


@pytest.mark.parametrize("name", NAMES)
def test_case_is_a_cholesky_shaped_tree_on_its_edge(name):
    case = SC.BY_NAME[name]
    n, Lp, Li, Lx, growth, M, launches = SC.built(name)
    assert Lp.dtype == np.int32 and Li.dtype == np.int32 and Lp[0] == 0 and Lp[n] == Li.size == Lx.size
    assert SC.is_cholesky_shaped(n, Lp, Li)
    par = SC.parent_of(n, Lp, Li)
    assert np.count_nonzero(par < 0) == 1 and n > 256         # one tree of more than 256 columns: no forest of small trees
    assert np.all(np.isfinite(Lx)) and np.all(Lx[Lp[:-1]] != 0.0)
    assert case.growth[0] < growth <= case.growth[1] or growth == 0.0 == case.growth[0]
    if case.path == 4:
        assert M is not None and M["kept"] and 8 * M["est_steps"] <= M["col_levels"]
        assert M["max_tree"] == n
    assert case.edge(M, launches)
    assert 1 <= min(case.ks) and len(set(case.ks)) == len(case.ks)


def test_is_cholesky_shaped_refuses_what_is_not():
    n, Lp, Li = SC.comb(4, 64, 8, 64, reach=3)
    assert SC.is_cholesky_shaped(n, Lp, Li)
    bad = Li.copy()
    j = 63                                   # the last column of the first leaf: swap one of its supernode rows for a root row
    bad[Lp[j] + 2] = n - 1
    bad[Lp[j] + 1:Lp[j + 1]] = np.sort(bad[Lp[j] + 1:Lp[j + 1]])
    assert not SC.is_cholesky_shaped(n, Lp, bad)
    unsorted = Li.copy()
    unsorted[Lp[j] + 1], unsorted[Lp[j] + 2] = Li[Lp[j] + 2], Li[Lp[j] + 1]
    assert not SC.is_cholesky_shaped(n, Lp, unsorted)


def test_every_kernel_family_and_rule_of_the_table_has_a_case():
    """over all cases and their batch sizes the expected launches name every kernel a solve can enqueue (k_sn_mfma<., false,
    1 | 4, 4> need a plan with chunks of 64 AND matrix-core fragments: the case whose bad block the 64-column ranges split)"""
    seen = set()
    for name in NAMES:
        case = SC.BY_NAME[name]
        M, launches = SC.built(name)[5:]
        if M is None:
            continue
        for k in case.ks:
            for d in ("fwd", "bwd"):
                seen |= {key for key, v in launches(k)[d].items() if v}
    assert seen == set(SC.LAUNCHES)
    # both sides of every threshold
    g = lambda name: SC.built(name)[5]
    assert {g(nm)["fwd"]["max_step_tasks"] for nm in ("step16384", "step16385")} == {SC.WG_TASKS, SC.WG_TASKS + 1}
    assert {g("leaf_tasks8191")["leaf_tasks"], g("leaf_tasks8192")["leaf_tasks"]} == {SC.THIN_TASKS - 1, SC.THIN_TASKS}
    assert {g(nm)["leaf_subtrees"] for nm in ("leaves256", "leaves257", "leaves512", "leaves513")} == {256, 257, 512, 513}
    assert g("guard_relaxed") is None and g("guard_fundamental")["chunk"] == 64
    assert {len(g(nm)["chunks"]) - 4 for nm in ("root127", "root128", "root129", "root256", "root257")} == {1, 2, 3}
