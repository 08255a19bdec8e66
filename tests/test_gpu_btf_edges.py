"""Every case of tests/btf_cases.py on the device: csx_btf_info as the model says; the structure of the factors; forward and
transposed solves byte-equal to btf_oracle.solve and trans_oracle.btf_solve_trans on the factor's own factors, every column of a
block of right-hand sides byte-equal to the list solve of that column, reruns equal, and the backward error of the device's x under
the bound the CPU test admits the case by; for the refactor cases L, U byte-equal to refactor_oracle.refactor on the kept patterns and
everything byte-equal to a fresh factor of the new values, and a failing refactor that changes nothing.  lusol_factor.refactor runs
the same kernel on disconnected dense components on each side of its cuts."""
import numpy as np
import pytest
import scipy.sparse as sp

import btf_cases as BC
import btf_oracle
import refactor_oracle as R
import trans_oracle as T
from test_gpu_btf import _cs, _sp, check_structure, cs
from test_gpu_refactor import _arr, _same_factors, _same_lu

pytestmark = pytest.mark.gpu


def _lists(M, n):
    """(p, i, x) of a factor as it is now, in lists of its own"""
    nnz = M.p[n]
    return list(M.p[:n + 1]), list(M.i[:nnz]), list(M.x[:nnz])


def _backward_error(S, x, b):
    return np.max(np.abs(S @ x - b)) / (abs(S).sum(axis=1).max() * np.max(np.abs(x)) + np.max(np.abs(b)))


def _list_solves(sol, S, seed):
    """forward and transposed list solves: the oracle's bytes on the solver's own factors, and a small backward error"""
    n = S.shape[0]
    f = sol.factors
    rng = np.random.default_rng(seed)
    out = []
    for trans in (False, True):
        b = rng.uniform(-1, 1, n)
        x = b.tolist()
        assert sol.solve(x, trans=trans) is True
        x = np.asarray(x)
        oracle = T.btf_solve_trans if trans else btf_oracle.solve
        want = np.asarray(oracle(f.L, f.U, f.F, f.pinv, f.p, f.q, f.r, b.tolist()))
        assert x.tobytes() == want.tobytes(), trans
        err = _backward_error(S.T.tocsc() if trans else S, x, b)
        print("backward error", "trans" if trans else "forward", err)
        assert err < BC.BOUND, (trans, err)      # (the oracle's figure, by the bytes: a wrong oracle must not hide a wrong kernel)
        out.append(x.tobytes())
    return out


def _block_solves(sol, n, widths, seed):
    """every column of a dvec solve is the list solve of that column; a second run gives the first one's bytes"""
    c = cs()
    rng = np.random.default_rng(seed)
    for trans in (False, True):
        for k in widths:
            B = rng.uniform(-1, 1, (n, k))
            dB = c.dvec(B)
            assert sol.solve(dB, trans=trans) is True
            X = dB.numpy().reshape(n, k)
            cols = range(k) if k <= BC.RHS_TILE + 1 else sorted(set(BC.WIDE_COLUMNS + (k - 1,)))
            for col in cols:
                xc = B[:, col].tolist()
                sol.solve(xc, trans=trans)
                assert np.asarray(xc).tobytes() == np.ascontiguousarray(X[:, col]).tobytes(), (trans, k, col)
            dB2 = c.dvec(B)
            sol.solve(dB2, trans=trans)
            assert dB2.numpy().tobytes() == X.tobytes(), (trans, k)


def _split(S2, f):
    """D and F of S2(p, q) with the factor's own p, q and blocks, as (p, i, x) lists"""
    return btf_oracle.split(S2.shape[0], S2.indptr.tolist(), S2.indices.tolist(), S2.data.tolist(), f.p.tolist(), f.q.tolist(),
                            f.r.tolist())


def _facts_of(sol, n):
    f = sol.factors
    info = sol.info()
    M = {"sizes": np.diff(f.r), "levels": np.asarray(f.levels), "fnz": info["fnz"], "n": n}
    tc = BC.term_counts(f.L, f.U, f.F, f.r)
    return info, BC.facts(M, tc), tc


def _block_in_factor_order(M, f):
    """rows, cols of the dense SMALL-row block (S's indices, dominant pairs aligned), and the places in cols of the last and the
    last but one column the factorisation takes in that block"""
    rows, cols = BC.block_of(M, True)
    qinv = np.empty(M["n"], np.int64)
    qinv[f.q] = np.arange(M["n"])
    pos = qinv[cols]
    b = int(np.searchsorted(f.r, pos.min(), side="right")) - 1
    r0, r1 = int(f.r[b]), int(f.r[b + 1])
    assert r1 - r0 == len(cols) and pos.min() == r0 and pos.max() == r1 - 1
    # the kept pivot of the column at position k is the dominant entry: row p[i] with pinv[i] == k is cols' partner in rows
    prow = np.empty(M["n"], np.int64)
    prow[f.pinv] = f.p                                         # position k -> A's row of its pivot
    assert np.array_equal(prow[pos], rows)
    return rows, cols, int(np.flatnonzero(pos == r1 - 1)[0]), int(np.flatnonzero(pos == r1 - 2)[0])


@pytest.mark.parametrize("name", list(BC.CASES))
def test_case_on_the_device(name):
    c = cs()
    case, M = BC.CASES[name], BC.get(name)
    S, n, tol = M["S"], M["n"], M["tol"]
    sol = c.btf_factor(_cs(S), tol)
    assert sol is not None
    f = sol.factors
    info, facts, tc = _facts_of(sol, n)
    want = BC.plan_model(M["sizes"], M["levels"], M["fnz"])
    for key in ("blocks", "levels", "max_block", "large_blocks", "launches", "fnz"):
        assert info[key] == want[key], (key, info[key], want[key])
    assert sorted(zip(np.asarray(f.levels).tolist(), np.diff(f.r).tolist())) == sorted(zip(M["levels"].tolist(), M["sizes"].tolist()))
    for key, value in case["claims"].items():
        if key in facts:
            assert facts[key] == value, (key, facts[key], value)
    BC.check_counts(case["claims"], tc)                        # on the factor's own L, U and F
    if case["claims"].get("pivots_move"):
        b = int(np.flatnonzero(np.diff(f.r) == BC.BTF_SMALL)[0])
        a, e = int(f.r[b]), int(f.r[b + 1])
        assert (np.asarray(f.pinv[a:e]) != np.arange(a, e)).sum() > BC.BTF_SMALL // 2
    check_structure(S, sol)
    first = _list_solves(sol, S, M["seed"])                    # (the transposed programs exist before any refactor)
    _block_solves(sol, n, M["widths"], M["seed"] + 1)
    if M["refactor"] is None:
        return
    L0, U0 = _lists(f.L, n), _lists(f.U, n)
    model = BC.refactor_model(np.diff(f.r))
    assert model == BC.refactor_model(M["sizes"])
    if M["refactor"] == "singular":
        rows, cols, last, prev = _block_in_factor_order(M, f)
        S2 = BC.singular_values(S, rows, cols, last, prev, M["seed"] + 1000)
        D2, _ = _split(S2, f)
        assert R.refactor(L0, U0, f.pinv, D2)[2] is False      # the rule itself stops at a zero pivot
        kept = [_arr(getattr(f, which), n)[2].tobytes() for which in ("L", "U", "F", "D")]
        assert sol.refactor(S2.data) is False
        rinfo = sol.refactor_info()
        assert rinfo["ok"] is False and rinfo["device_columns"] == model["device_columns"] and rinfo["host_columns"] == 0
        assert [_arr(getattr(f, which), n)[2].tobytes() for which in ("L", "U", "F", "D")] == kept
        assert _list_solves(sol, S, M["seed"]) == first
        _block_solves(sol, n, (BC.RHS_TILE + 1,), M["seed"] + 1)
        # (and the solver is as good as new: the refactor below runs on the maps and the schedule the failed one built)
    S2 = BC.perturbed(S, M["seed"] + 1000)
    assert sol.refactor(_cs(S2)) is True
    rinfo = sol.refactor_info()
    assert (rinfo["device_columns"], rinfo["host_columns"]) == (model["device_columns"], model["host_columns"])
    assert 0.0 < rinfo["pivot_ratio"] <= 1.0
    D2, F2 = _split(S2, f)
    Lx, Ux, ok, ratio = R.refactor(L0, U0, f.pinv, D2)
    assert ok and ratio == rinfo["pivot_ratio"]
    assert _arr(f.L, n)[2].tobytes() == np.asarray(Lx).tobytes()
    assert _arr(f.U, n)[2].tobytes() == np.asarray(Ux).tobytes()
    for got, split in ((f.D, D2), (f.F, F2)):                  # the values of A2, entry for entry
        assert (_sp(got, n) != sp.csc_matrix((split[2], split[1], split[0]), shape=(n, n))).nnz == 0
    fresh = c.btf_factor(_cs(S2), tol)
    _same_factors(f, fresh.factors, n)
    second = _list_solves(sol, S2, M["seed"])
    assert second != first
    _block_solves(sol, n, (1, BC.RHS_TILE + 1), M["seed"] + 2)
    assert sol.condest() == fresh.condest()
    assert sol.refactor(_cs(S)) is True                        # and back: the first bytes again
    assert _list_solves(sol, S, M["seed"]) == first


def test_lusol_refactor_on_dense_components():
    c = cs()
    S, S2, sizes = BC.lusol_components()
    n = S.shape[0]
    model = BC.refactor_model(sizes)
    sol = c.lusol_factor(_cs(S), 0, 1.0, exact=True)
    N = sol.factors
    L0, U0 = _lists(N.L, n), _lists(N.U, n)
    B = np.random.default_rng(5).uniform(-1, 1, (n, BC.RHS_TILE + 1))
    for trans in (False, True):
        sol.solve(c.dvec(B), trans=trans)                      # plans exist before the refactor: they must be rebuilt
    assert sol.refactor(_cs(S2)) is True
    info = sol.refactor_info()
    assert (info["device_columns"], info["host_columns"]) == (model["device_columns"], model["host_columns"])
    Lx, Ux, ok, ratio = R.refactor(L0, U0, N.pinv, (S2.indptr.tolist(), S2.indices.tolist(), S2.data.tolist()))
    assert ok and ratio == info["pivot_ratio"] and 0.0 < ratio <= 1.0
    assert _arr(N.L, n)[2].tobytes() == np.asarray(Lx).tobytes()
    assert _arr(N.U, n)[2].tobytes() == np.asarray(Ux).tobytes()
    fresh = c.lusol_factor(_cs(S2), 0, 1.0, exact=True)
    _same_lu(sol, fresh, n)
    for trans in (False, True):
        d1, d2 = c.dvec(B), c.dvec(B)
        sol.solve(d1, trans=trans)
        fresh.solve(d2, trans=trans)
        assert d1.numpy().tobytes() == d2.numpy().tobytes()
        x = d1.numpy().reshape(n, -1)[:, 0]
        assert _backward_error(S2.T.tocsc() if trans else S2, x, B[:, 0]) < BC.BOUND
