"""The assembly plan without a GPU (include/csx.h, "assembly plan"): the pure-Python restatement of its
definition against the oracle's cs_dupl(cs_compress(T)), the library's host rule against the restatement, and the
declarations.  Every comparison of values is byte equality."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import assemble_oracle as AO
import csparse_oracle as PO
from conftest import ROOT

CASES = [(name, split) for name in AO.GOLDEN_WITH_TRIPLETS for split in (False, True)]
ENTRY_POINTS = {"csx_assemble_plan_host": 10, "csx_assemble_host": 5, "csx_assemble_plan": 6, "csx_assemble_matrix": 3,
                "csx_assemble": 3, "csx_assemble_plan_info": 2}


def check_restatement(m, n, Ti, Tj, Tx, Cref):
    p, i, sp, src = AO.plan(m, n, Ti, Tj)
    nnz = p[n]
    assert p == Cref.p and i == Cref.i[:nnz] and len(Cref.i) == nnz
    assert sorted(src) == list(range(len(Ti))) and sp[0] == 0 and sp[-1] == len(Ti) and len(sp) == nnz + 1
    assert all(src[t] < src[t + 1] for s in range(nnz) for t in range(sp[s], sp[s + 1] - 1))
    assert AO.as_bytes(AO.fold(sp, src, Tx)) == AO.as_bytes(Cref.x[:nnz])
    return p, i, sp, src


@pytest.mark.parametrize("name,split", CASES, ids=["%s-%s" % (c[0], "split" if c[1] else "plain") for c in CASES])
def test_restatement_matches_oracle_on_golden(name, split):
    m, n, Ti, Tj, Tx, Cref = AO.golden_case(name, split)
    p, i, sp, src = check_restatement(m, n, Ti, Tj, Tx, Cref)
    if split:
        assert min(sp[s + 1] - sp[s] for s in range(p[n])) >= 3   # every slot has duplicates


@pytest.mark.parametrize("case", AO.random_cases(), ids=lambda c: c[0])
def test_restatement_matches_oracle_on_random_and_edges(case):
    label, m, n, Ti, Tj, Tx = case
    Cref = AO.composite(PO, m, n, Ti, Tj, Tx)
    p, i, sp, src = check_restatement(m, n, Ti, Tj, Tx, Cref)
    if label.startswith("wide"):
        # the comparison can tell a wrong order from the right one
        assert AO.as_bytes(AO.fold(sp, src, Tx, reverse=True)) != AO.as_bytes(Cref.x[:p[n]])
    if label == "negzero":
        x = AO.fold(sp, src, Tx)
        assert AO.as_bytes(x) == AO.as_bytes([-0.0, 0.0, -0.0])
        assert AO.as_bytes([0.0 + -0.0 + -0.0]) != AO.as_bytes([-0.0])   # why the first term is assigned


def host_plan(lib, m, n, Ti, Tj):
    import _csx
    nz = len(Ti)
    ti, tj = _csx.i32(Ti), _csx.i32(Tj)
    Cp, Ci = np.full(n + 1, -7, np.int32), np.full(max(nz, 1), -7, np.int32)
    sp, src = np.full(nz + 1, -7, np.int32), np.full(max(nz, 1), -7, np.int32)
    nnz = C.c_int32(-1)
    st = lib.csx_assemble_plan_host(m, n, nz, _csx.pi(ti), _csx.pi(tj), _csx.pi(Cp), _csx.pi(Ci), _csx.pi(sp), _csx.pi(src), nnz)
    return st, Cp, Ci, sp, src, nnz.value


def check_host_abi(m, n, Ti, Tj, Tx):
    import _csx
    lib = _csx.load()
    p, i, sp, src = AO.plan(m, n, Ti, Tj)
    st, Cp, Ci, hsp, hsrc, nnz = host_plan(lib, m, n, Ti, Tj)
    assert st == _csx.OK and nnz == p[n]
    assert Cp.tolist() == p and Ci[:nnz].tolist() == i
    assert hsp[:nnz + 1].tolist() == sp and hsrc[:len(Ti)].tolist() == src
    tx = _csx.f64(Tx)
    out = np.full(max(nnz, 1), np.nan)
    assert lib.csx_assemble_host(nnz, _csx.pi(hsp), _csx.pi(hsrc), _csx.pd(tx), _csx.pd(out)) == _csx.OK
    assert out[:nnz].tobytes() == AO.as_bytes(AO.fold(sp, src, Tx))


@pytest.mark.parametrize("name,split", CASES, ids=["%s-%s" % (c[0], "split" if c[1] else "plain") for c in CASES])
def test_host_abi_matches_restatement_on_golden(name, split):
    m, n, Ti, Tj, Tx, _ = AO.golden_case(name, split)
    check_host_abi(m, n, Ti, Tj, Tx)


@pytest.mark.parametrize("case", AO.random_cases(), ids=lambda c: c[0])
def test_host_abi_matches_restatement_on_random_and_edges(case):
    check_host_abi(*case[1:])


def test_host_abi_refuses_an_index_out_of_range():
    import _csx
    lib = _csx.load()
    for Ti, Tj in (([0, 3], [0, 1]), ([0, -1], [0, 1]), ([0, 1], [0, 2]), ([0, 1], [-1, 1])):
        assert host_plan(lib, 3, 2, Ti, Tj)[0] == _csx.EINVAL
        with pytest.raises(IndexError):
            AO.plan(3, 2, Ti, Tj)
    assert host_plan(lib, 3, 2, [2, 0], [1, 0])[0] == _csx.OK


def test_host_abi_refuses_more_triplets_than_int32_holds():
    """nz > 2^31 - 1 is refused before any array is read (the arrays here have one entry)"""
    import _csx
    lib = _csx.load()
    one = [np.zeros(1, np.int32) for _ in range(6)]
    nnz = C.c_int32(-1)
    for nz, want in ((2 ** 31, _csx.EINVAL), (-1, _csx.EINVAL), (1, _csx.OK)):
        assert lib.csx_assemble_plan_host(1, 1, nz, *[_csx.pi(a) for a in one[:2]], _csx.pi(np.zeros(2, np.int32)),
                                          _csx.pi(one[3]), _csx.pi(np.zeros(2, np.int32)), _csx.pi(one[5]), nnz) == want
    assert nnz.value == 1


def test_header_declares_and_csx_binds_the_entry_points():
    import _csx
    text = open(os.path.join(ROOT, "include", "csx.h")).read()
    assert "assembly plan" in text and "The first term is ASSIGNED" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _csx.load()
    for name, arity in ENTRY_POINTS.items():
        decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert decl, name
        assert len(decl.group(1).split(",")) == arity == len(_csx._PROTOS[name]), name
        assert hasattr(lib, name), name
