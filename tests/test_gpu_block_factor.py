"""The block routes of cs_lu and cs_qr (csx_lu_blocks, csx_qr_blocks), the connected-components pass under them, the strip-to-CSC
fill and csx_happly on the device, over the table of tests/block_cases.py: every size cut, membership shape, pivot tie, storage
order, singular column, cs_house branch and csx_happly route (needs an MI355X).  Everything is compared as bytes -- L, U, pinv, V,
R, beta with the host code the device route restates (csx_lu_host, pinned to the oracle in tests/test_block_cases_cpu.py;
csx_qr_host), csx_happly with the oracle's cs_happly applied reflection by reflection, the components with a union-find -- and the
only tolerance is the residual bound of tests/test_gpu_lu_blocks.py."""
import numpy as np
import pytest

import block_cases as BC
import c_oracle as CO
import csparse_oracle as O
from test_gpu_parity import _host_cs, cs  # noqa: F401
from test_gpu_qr_device import _qr_both_ways
from test_lu_oracle import host_lu

pytestmark = pytest.mark.gpu


def _lu_matches_host(cs, M, tol, route):
    n, Ap, Ai, Ax = M["n"], M["Ap"], M["Ai"], M["Ax"]
    A = cs.cs_pin(_host_cs(cs, n, n, Ap, Ai, Ax))
    N = cs.cs_lu(A, cs.cs_sqr(0, A, False), tol)
    assert N is not None and bool(N.L._lazy) == (route == "device")
    Lp, Li, Lx, Up, Ui, Ux, pinv = host_lu(n, Ap, Ai, Ax, tol)
    nl, nu = int(Lp[n]), int(Up[n])
    assert N.pinv == pinv.tolist()
    assert N.L.p == Lp.tolist() and N.U.p == Up.tolist()
    assert N.L.i[:nl] == Li.tolist() and N.U.i[:nu] == Ui.tolist()
    assert np.asarray(N.L.x[:nl]).tobytes() == Lx.tobytes() and np.asarray(N.U.x[:nu]).tobytes() == Ux.tobytes()
    # the factors solve the system (of the last stored value where a column stores a row twice)
    Ep, Ei, Ex = BC.last_wins(M)
    b = 1.0 + np.arange(n) / n
    bl = b.tolist()
    assert cs.cs_lusol(0, A, bl, tol) is True
    xs = np.asarray(bl)
    res = CO.gaxpy(n, n, Ep, Ei, Ex, xs, -b)
    norm1 = float(np.max(np.add.reduceat(np.abs(Ex), Ep[:-1])))
    assert np.max(np.abs(res)) <= 1e-12 * (norm1 * np.max(np.abs(xs)) + np.max(np.abs(b)))


@pytest.mark.parametrize("name,tol", BC.LU_CASES)
def test_lu_blocks_bit_identical_to_host_code(cs, name, tol):
    _lu_matches_host(cs, BC.get(name), tol, BC.CASES[name]["claims"]["route"])


@pytest.mark.parametrize("name", BC.SINGULAR_CASES)
def test_lu_blocks_singular_block_gives_none_and_the_next_call_is_right(cs, name):
    M = BC.get(name)
    n = M["n"]
    A = cs.cs_pin(_host_cs(cs, n, n, M["Ap"], M["Ai"], M["Ax"]))
    assert cs.cs_lu(A, cs.cs_sqr(0, A, False), 1.0) is None
    b = (1.0 + np.arange(n) / n).tolist()
    kept = list(b)
    assert cs.cs_lusol(0, A, b, 1.0) is False and b == kept
    healthy, tol = BC.HEALTHY_AFTER_SINGULAR
    _lu_matches_host(cs, BC.get(healthy), tol, "device")


@pytest.mark.parametrize("name", BC.QR_CASES)
def test_qr_blocks_bit_identical_to_host_code(cs, name):
    M = BC.get(name)
    n, Ap, Ai, Ax = M["n"], M["Ap"], M["Ai"], M["Ax"]
    if BC.CASES[name]["claims"]["route"] == "device":
        _qr_both_ways(cs, n, Ap, Ai, Ax)                                  # V, R, beta as bytes, and N.L._lazy
    else:
        A = cs.cs_pin(_host_cs(cs, n, n, Ap, Ai, Ax))
        S = cs.cs_sqr(0, A, True)
        N = cs.cs_qr(A, S)
        assert S.m2 == n and N is not None and not N.L._lazy              # done = 0: the host code


_FACTORS = {}


def _happly_factor(cs, name):
    if name not in _FACTORS:
        M = BC.happly_matrix(name)
        A = _host_cs(cs, M["n"], M["n"], M["Ap"], M["Ai"], M["Ax"])
        N = cs.cs_qr(A, cs.cs_sqr(0, A, True))
        assert N is not None and N.L.m == M["n"]
        oV = O.cs_spalloc(N.L.m, N.L.n, len(N.L.i), True, False)
        oV.p, oV.i, oV.x = list(N.L.p), list(N.L.i), list(N.L.x)
        _FACTORS[name] = (N, oV)
    return _FACTORS[name]


@pytest.mark.parametrize("nrhs", BC.HAPPLY_NRHS)
@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("name", list(BC.HAPPLY_CASES))
def test_happly_routes_bit_identical_to_the_oracle(cs, name, transpose, nrhs):
    N, oV = _happly_factor(cs, name)
    n, m2 = N.L.n, N.L.m
    B = np.random.default_rng(7).uniform(-1, 1, size=(m2, nrhs))
    X = cs.dvec(B)
    assert cs.apply_q(N, X, transpose) is True
    got = X.numpy().reshape(m2, nrhs)
    for r in sorted(set(c for c in BC.HAPPLY_COLUMNS + (nrhs - 1,) if c < nrhs)):
        x = B[:, r].tolist()
        for t in range(n):
            i = t if transpose else n - 1 - t
            O.cs_happly(oV, i, N.B[i], x)
        assert got[:, r].tobytes() == np.asarray(x).tobytes(), (name, transpose, nrhs, r)


@pytest.mark.parametrize("name", list(BC.COMPONENT_CASES))
def test_components_against_union_find(cs, name):
    import _csx
    n, Ap, Ai, sf, sl, order, malformed = BC.component_case(name)
    out = _csx.prim_components(n, Ap, Ai, sf, sl, order)
    assert out["malformed"] == (1 if malformed else 0)
    assert out["p"].tobytes() == Ap.tobytes() and out["i"].tobytes() == Ai.tobytes()      # the device copies are as they came
    if malformed:
        return
    root = BC.roots(n, Ap, Ai, sf, sl)                                    # the smallest vertex of every component
    nodes, first, count, comp_of_pos, ncomp, maxc = BC.grouping(root)
    assert (out["ncomp"], out["maxc"]) == (ncomp, maxc)
    assert out["root"].tobytes() == root.tobytes()
    assert out["nodes"].tobytes() == nodes.tobytes()                      # grouped by root, ascending inside a group
    assert out["first"].tobytes() == first.tobytes() and out["count"].tobytes() == count.tobytes()
    assert out["comp_of_pos"].tobytes() == comp_of_pos.tobytes()
