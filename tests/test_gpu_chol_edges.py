"""The general cs_chol numeric (csx_chol.hip, chol_analysis_run) on the constructed cases of
tests/chol_cases.py: every k_chol_band instance on both sides of its class, the in-place branch of chol_column, the wave split
and the row map of k_chol_coop, the two-phase run rule, the small-tree and dense-tree limits and chol_supernodes' panels.  A
fresh cs_chol and a refactor of both congruent value sets are held to the plain-C oracle: pattern equal, L.x byte for byte on
the exact routes (register window, blocked band, dense trees) and within tol.CHOL_EPS_UNITS roundings of an entry's terms on
the rounding routes (a bound taken from the oracle's own distance to a longdouble factor, not from the device); the route the
case is named for is read back (refactor_info(): band kind, the window that ran, supernodes, trees, the model's launch count),
the rounding routes give the same bytes twice, and a matrix that is not positive definite is refused and changes nothing.
tests/test_chol_cases_cpu.py shows without a device that every case sits on its edge and that no update is small enough to
hide inside the bound."""
import numpy as np
import pytest

import chol_cases as CC
import tol as TOL
from test_gpu_chol_refactor import _device_arrays, _options
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu


def _hold(name, which, p, i, x, what):
    """L (p, i, x) against the oracle's factor of the case's value set `which`"""
    case = CC.BY_NAME[name]
    Lp, Li, Lx = CC.oracle(name, which)
    n, lnz = case.n, int(Lp[case.n])
    assert np.array_equal(np.asarray(p, np.int64), Lp) and np.array_equal(np.asarray(i[:lnz], np.int64), Li), (name, what)
    x = np.asarray(x[:lnz], np.float64)
    cut = int(Lp[case.bytes_upto])
    assert x[:cut].tobytes() == Lx[:cut].tobytes(), (name, what, "an exact route differs from the oracle")
    if cut < lnz:
        units = CC.rounding_units(name, which, x)
        print("%s %s: %.2f eps units of the terms (bound %.2f)" % (name, what, units, TOL.CHOL_EPS_UNITS))
        assert units <= TOL.CHOL_EPS_UNITS, (name, what, units)
    return x


def _fresh(cs, case, x):
    A = case.matrix(cs, x)
    return cs.cs_chol(A, cs.cs_schol(0, A))


@pytest.mark.parametrize("name", CC.NAMES)
def test_fresh_factor_equals_the_oracle(cs, name):
    case = CC.BY_NAME[name]
    lnz = int(CC.oracle(name)[0][case.n])
    with _options(case):
        N = _fresh(cs, case, case.x)
        assert N is not None
        x = _hold(name, "A", N.L.p, N.L.i, N.L.x, "fresh")
        if case.bytes_upto < case.n:                      # k_chol_coop's promise: the same bits every run
            again = np.asarray(_fresh(cs, case, case.x).L.x[:lnz])
            assert again.tobytes() == x.tobytes(), name


@pytest.mark.parametrize("name", CC.NAMES)
def test_refactor_equals_the_oracle_on_the_route_the_case_is_named_for(cs, name):
    case = CC.BY_NAME[name]
    with _options(case):
        F = cs.cholsol_factor(case.matrix(cs), 0)
        assert F is not None
        for k in (0, 1):
            assert F.refactor(case.A2[k]) is True
            p, i, x = _device_arrays(F)
            x = _hold(name, k, p, i, x, "refactor %d" % k)
            info = F.refactor_info(window=True)
            assert info["ok"] is True
            for key, want in case.expect.items():
                assert info[key] == want, (name, key, info)
            assert info["levels"] == CC.expected_levels(name), (name, info, CC.model(name)["launches"])
            if case.bytes_upto < case.n:
                assert F.refactor(case.A2[k]) is True
                assert _device_arrays(F)[2].tobytes() == x.tobytes(), (name, k)


@pytest.mark.parametrize("name", CC.NAMES)
def test_not_positive_definite_is_refused_and_changes_nothing(cs, name):
    case = CC.BY_NAME[name]
    with _options(case):
        F = cs.cholsol_factor(case.matrix(cs), 0)
        before = _device_arrays(F)[2].tobytes()
        for j in case.bad_at:
            bad = case.bad_values(j)
            assert _fresh(cs, case, bad) is None, (name, j)
            assert F.refactor(bad) is False, (name, j)
            assert F.refactor_info()["ok"] is False
            assert _device_arrays(F)[2].tobytes() == before, (name, j)


@pytest.mark.parametrize("name", [c.name for c in CC.CASES if c.twin])
def test_supernodes_on_and_off_agree(cs, name):
    """the clique of a hub through chol_supernodes and as a two-phase chain of k_chol_coop: two roundings of one factor"""
    case, twin = CC.BY_NAME[name], CC.BY_NAME[CC.BY_NAME[name].twin]
    assert case.x.tobytes() == twin.x.tobytes()
    lnz = int(CC.oracle(name)[0][case.n])
    got = []
    for c in (case, twin):
        with _options(c):
            got.append(np.asarray(_fresh(cs, c, c.x).L.x[:lnz]))
    units = float(np.max(np.abs(got[0] - got[1]) / (TOL.EPS * CC.terms(name, "A"))))
    print("%s against %s: %.2f eps units of the terms" % (name, twin.name, units))
    assert units <= TOL.CHOL_EPS_UNITS


def test_the_window_is_read_from_the_plan(cs):
    import _csx
    case = CC.BY_NAME["band47"]
    with _options(case):
        F = cs.cholsol_factor(case.matrix(cs), 0)
        assert F.refactor_info(window=True) is None
        assert F.refactor(case.A2[0]) is True
        assert "window" not in F.refactor_info() and F.refactor_info(window=True)["window"] == CC.WINDOWS[0]
        assert _csx.lib().csx_chol_refactor_window(F._rplan, None) == _csx.EINVAL
        out = _csx.C.c_int32(-1)
        assert _csx.lib().csx_chol_refactor_window(F.L._dev.handle, out) == _csx.EINVAL and out.value == -1   # not a plan
