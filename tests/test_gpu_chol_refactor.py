"""refactor() of cholsol_factor on the device: new values on the kept analysis give L.x byte-equal to a fresh
factor of the new values on every route (small trees, level lists with supernodes, both band kernels, two-phase chains, forests
of cliques and of small sparse trees, duplicates), the solves follow, a matrix that is not positive definite changes nothing and
another pattern is refused.  The inputs are tests/chol_refactor_cases.py (held to their assumptions by
tests/test_chol_refactor_cases_cpu.py)."""
import contextlib
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import chol_refactor_cases as RC
import csparse_oracle as O
import tol as TOL
from test_gpu_parity import cs  # noqa: F401

pytestmark = pytest.mark.gpu

SOLVE_CASES = ["bcsstk01-ordered", "grid22", "grid24", "grid24nat", "grid24nat-coop", "cliques16-exact", "ragged", "sparse_trees",
               "dups"]


@contextlib.contextmanager
def _options(case):
    import _csx
    with contextlib.ExitStack() as stack:
        for name, value in case.options:
            stack.enter_context(_csx.option(name, value))
        yield


def _factor(cs, case, x=None):
    F = cs.cholsol_factor(case.matrix(cs, x), case.order, case.exact)
    assert F is not None
    return F


def _device_arrays(F):
    """L.p, L.i, L.x as they stand on the device"""
    import _csx
    dev = F.L._dev
    m, n, nnz, hv = dev.info()
    p, i, x = np.empty(n + 1, np.int32), np.empty(max(nnz, 1), np.int32), np.empty(max(nnz, 1), np.float64)
    _csx.check(_csx.lib().csx_csc_download(dev.handle, _csx.pi(p), _csx.pi(i), _csx.pd(x)), "csx_csc_download")
    return p, i[:nnz], x[:nnz]


def _Lx(F):
    return _device_arrays(F)[2].tobytes()


_FRESH = {}


def _fresh_Lx(cs, case, which):
    """L.x of a fresh cholsol_factor of the case's value set `which`, under the case's options (in force at the call); once"""
    key = (case.name, which)
    if key not in _FRESH:
        _FRESH[key] = _Lx(_factor(cs, case, case.x if which == "A" else case.A2[which]))
    return _FRESH[key]


def _same_factor(case, got, want):
    """L.x (bytes) against a fresh factor's: byte for byte, or -- the cases marked same_bytes=False, "chol.exact" = 0 with an
    emitting fresh factor -- within the 1e-10 that option grants L.x; the figure is printed either way"""
    if got != want:
        a, b = np.frombuffer(got), np.frombuffer(want)
        print("%s: L.x differs from the fresh factor's by %.3e (normwise)" % (case.name, TOL.normwise(a, b)))
    if case.same_bytes:
        return got == want
    return TOL.normwise(np.frombuffer(got), np.frombuffer(want)) < TOL.X_RTOL


def _check_info(case, info, first):
    assert info["ok"] is True and info["first"] is first
    assert set(info) == {"ok", "route", "levels", "supernodes", "trees", "dense_trees", "band", "first", "numeric_ms", "ms"}
    for key, want in case.expect.items():
        if want == ">=1":
            assert info[key] >= 1, (key, info)
        else:
            assert info[key] == want, (key, info)
    assert info["numeric_ms"] >= 0.0 and info["ms"] > 0.0


def _oracle_S(F):
    sym = F.symbolic
    S = O.css()
    S.parent, S.cp, S.pinv = list(sym.parent), list(sym.cp), None if sym.pinv is None else list(sym.pinv)
    S.lnz = S.unz = S.cp[-1]
    return S


@pytest.mark.parametrize("name", RC.NAMES)
def test_refactor_equals_a_fresh_factor_byte_for_byte(cs, name):
    case = RC.BY_NAME[name]
    with _options(case):
        F = _factor(cs, case)
        assert F.refactor_info() is None
        p0, i0, _ = _device_arrays(F)
        S = _oracle_S(F)
        for k, x2 in enumerate(case.A2):
            assert F.refactor(case.matrix(cs, x2)) is True
            p, i, x = _device_arrays(F)
            assert p.tobytes() == p0.tobytes() and i.tobytes() == i0.tobytes()
            assert _same_factor(case, x.tobytes(), _fresh_Lx(cs, case, k)), (name, k)
            _check_info(case, F.refactor_info(), k == 0)
            ref = RC.oracle_factor(O, case, k, S)
            assert ref is not None and np.array_equal(ref[0], p) and np.array_equal(ref[1], i)
            assert TOL.normwise(x, ref[2]) < TOL.X_RTOL
            big = np.abs(ref[2]) > 1e-6 * np.max(np.abs(ref[2]))
            assert np.max(np.abs(x[big] - ref[2][big]) / np.abs(ref[2][big])) < TOL.X_RTOL


@pytest.mark.parametrize("name", RC.NAMES)
def test_round_trip_restores_the_first_factor(cs, name):
    case = RC.BY_NAME[name]
    with _options(case):
        F = _factor(cs, case)
        x0 = _Lx(F)
        host_before = list(F.L.x)                           # host lists already read from F.L follow a refactor
        assert F.refactor(case.A2[0]) is True
        assert _Lx(F) != x0
        assert np.asarray(F.L.x[:len(host_before)]).tobytes() != np.asarray(host_before).tobytes()
        assert F.refactor(case.matrix(cs, case.A2[1])) is True
        assert F.refactor(case.x) is True
        assert _same_factor(case, _Lx(F), x0)
        assert _same_factor(case, np.asarray(F.L.x[:len(host_before)]).tobytes(), np.asarray(host_before).tobytes())


@pytest.mark.parametrize("name", SOLVE_CASES)
@pytest.mark.parametrize("exact", [None, True])
def test_solves_after_a_refactor(cs, name, exact):
    """exact=None and exact=True: the orders in which a list is solved as cs_cholsol solves it"""
    case = RC.BY_NAME[name]
    n = case.n
    rng = np.random.default_rng(5)
    with _options(case):
        F = cs.cholsol_factor(case.matrix(cs), case.order, exact)
        b = rng.uniform(-1.0, 1.0, n)
        x = b.tolist()
        assert F.solve(x) is True                           # a plan exists now, of the old values: it must be rebuilt
        old = np.asarray(x).tobytes()
        blk = cs.dvec(rng.uniform(-1.0, 1.0, (n, 3)))
        F.solve(blk)
        A2 = case.matrix(cs, case.A2[0])
        assert F.refactor(A2) is True
        x = b.tolist()
        assert F.solve(x) is True
        want = b.tolist()
        assert cs.cs_cholsol(case.order, case.matrix(cs, case.A2[0]), want) is True
        assert np.asarray(x).tobytes() == np.asarray(want).tobytes() != old
        for k in (1, 3, 70):
            B = rng.uniform(-1.0, 1.0, (n, k))
            dB = cs.dvec(B)
            assert F.solve(dB) is True
            X = dB.numpy().reshape(n, k)
            for c in range(k):
                col = B[:, c].tolist()
                F.solve(col)
                assert TOL.normwise(X[:, c], col) < TOL.X_RTOL, (k, c)
                if exact is True:
                    assert X[:, c].tobytes() == np.asarray(col).tobytes(), (k, c)


@pytest.mark.parametrize("name", RC.NAMES)
def test_not_positive_definite_changes_nothing(cs, name):
    case = RC.BY_NAME[name]
    b = np.random.default_rng(6).uniform(-1.0, 1.0, case.n)
    with _options(case):
        F = _factor(cs, case)
        x0 = _Lx(F)
        s0 = b.tolist()
        F.solve(s0)
        assert F.refactor(case.bad) is False
        assert F.refactor_info()["ok"] is False
        assert _Lx(F) == x0
        s1 = b.tolist()
        F.solve(s1)
        assert np.asarray(s1).tobytes() == np.asarray(s0).tobytes()
        assert F.refactor(case.matrix(cs, case.bad)) is False and _Lx(F) == x0
        assert F.refactor(case.matrix(cs, case.A2[0])) is True
        assert _same_factor(case, _Lx(F), _fresh_Lx(cs, case, 0))
        assert F.refactor_info()["ok"] is True and F.refactor_info()["first"] is False


@pytest.mark.parametrize("name", ["grid24", "cliques16-exact"])
def test_another_pattern_is_refused_and_every_input_kind_agrees(cs, name):
    case = RC.BY_NAME[name]
    with _options(case):
        F = _factor(cs, case)
        x0 = _Lx(F)
        moved = case.matrix(cs, case.A2[0])
        last = int(case.p[1]) - 1 if name == "cliques16-exact" else int(case.p[case.n]) - 3
        rows = list(moved.i)
        rows[last] = rows[last] + 1 if name == "cliques16-exact" else rows[last] - 1   # one entry moved to a row the column lacks
        moved.i = rows
        with pytest.raises(ValueError):
            F.refactor(moved)
        with pytest.raises(ValueError):
            F.refactor(case.A2[0][:-1])
        with pytest.raises(ValueError):
            F.refactor(cs.dvec(np.append(case.A2[0], 1.0)))
        assert _Lx(F) == x0 and F.refactor_info() is None
        got = []
        for A2 in (case.matrix(cs, case.A2[0]), case.A2[0].copy(), case.A2[0].tolist(), cs.dvec(case.A2[0])):
            assert F.refactor(case.A2[1]) is True           # away from the values under test
            assert F.refactor(A2) is True
            got.append(_Lx(F))
        assert got[0] == got[1] == got[2] == got[3] == _fresh_Lx(cs, case, 0)


@pytest.mark.parametrize("name", ["grid24", "grid24nat", "cliques16-exact", "sparse_trees"])
def test_update_then_refactor_and_the_readers_of_L(cs, name):
    case = RC.BY_NAME[name]
    n = case.n
    with _options(case):
        F = _factor(cs, case)
        x0 = _Lx(F)
        Cm = cs.cs_spalloc(n, 1, 1, True, False)            # one column with one entry: inside the pattern of L(:, f)
        Cm.p, Cm.i, Cm.x = [0, 1], [n // 3], [0.5]
        assert F.update(Cm) is True
        assert _Lx(F) != x0
        assert F.refactor(case.matrix(cs, case.A2[0])) is True
        assert _Lx(F) == _fresh_Lx(cs, case, 0)
        G = _factor(cs, case, case.A2[0])
        assert F.inverse_diag().tobytes() == G.inverse_diag().tobytes()
        assert abs(F.logdet() - G.logdet()) <= 1e-12 * abs(G.logdet())
        dense = case.effective_upper(case.A2[0])
        dense = dense + np.triu(dense, 1).T
        assert abs(F.logdet() - np.linalg.slogdet(dense)[1]) <= 1e-10 * abs(G.logdet())


def _upload(p, i, x, n):
    import _csx
    h = _csx.new_handle()
    _csx.check(_csx.lib().csx_csc_upload(n, n, _csx.pi(_csx.i32(p)), _csx.pi(_csx.i32(i)), _csx.pd(_csx.f64(x)), h), "csx_csc_upload")
    return h


def test_c_abi(cs):
    import _csx
    lib = _csx.lib()
    case = RC.BY_NAME["grid24nat"]
    n = case.n
    F = _factor(cs, case)
    hL = F.L._dev.handle
    x0 = _Lx(F)
    # an upper entry (0, n - 1) outside the band of L: no slot
    p, i, x = case.p.copy(), case.i.tolist(), case.x.tolist()
    at = int(p[n - 1])
    i.insert(at, 0)
    x.insert(at, -0.25)
    p[n] += 1
    hBad = _upload(p, i, x, n)
    plan = _csx.new_handle()
    assert lib.csx_chol_refactor_plan(hBad, hL, None, plan) == _csx.EINVAL
    assert "no slot in L" in lib.csx_last_error().decode()
    _csx.free(hBad)
    # a matrix that is not Cholesky-shaped in L's place
    hA = _upload(case.p, case.i, case.x, n)
    assert lib.csx_chol_refactor_plan(hA, hA, None, plan) == _csx.EINVAL
    assert "Cholesky-shaped" in lib.csx_last_error().decode()
    _csx.check(lib.csx_chol_refactor_plan(hA, hL, None, plan), "csx_chol_refactor_plan")
    ok, info = C.c_int(7), np.full(8, -1, np.int32)
    short = cs.dvec(case.A2[0][:-1])
    _csx.check(lib.csx_chol_refactor(plan, short.handle, ok, _csx.pi(info)), "csx_chol_refactor")
    assert ok.value == -1 and _Lx(F) == x0
    good = cs.dvec(case.A2[0])
    _csx.check(lib.csx_chol_refactor(plan, good.handle, ok, _csx.pi(info)), "csx_chol_refactor")
    assert ok.value == 1 and info.tolist() == [0, 0, 0, 0, 0, 1, 1, 0]
    assert _Lx(F) == _fresh_Lx(cs, case, 0)
    _csx.check(lib.csx_chol_refactor(plan, good.handle, ok, None), "csx_chol_refactor")   # info may be NULL
    num, call = C.c_double(-1.0), C.c_double(-1.0)
    _csx.check(lib.csx_chol_refactor_info(num, call), "csx_chol_refactor_info")
    assert 0.0 <= num.value <= call.value
    _csx.free(plan)                                           # the plan goes before L: L is still whole
    _csx.free(hA)
    assert _Lx(F) == _fresh_Lx(cs, case, 0)
    b = [1.0] * n
    assert F.solve(b) is True


def test_refactor_info_before_the_first_refactor():
    """csx_chol_refactor_info answers CSX_EINVAL until a csx_chol_refactor has run: process-wide state, so asked of a new process"""
    import _csx
    pkg = os.path.dirname(os.path.abspath(_csx.__file__))
    code = ("import ctypes as C, _csx\n"
            "a, b = C.c_double(0.0), C.c_double(0.0)\n"
            "print('status', _csx.lib().csx_chol_refactor_info(a, b) == _csx.EINVAL)\n")
    env = dict(os.environ, PYTHONPATH=pkg + os.pathsep + os.environ.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    assert "status True" in out.stdout
