"""The Dulmage-Mendelsohn oracle of the GPU tests (dm_oracle.py), pinned without a device: the reference test file's
known answers on its ten matrices, scipy's structural rank and strongly connected components; and cs_randperm,
which needs no device."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse import csgraph

import dm_oracle
from conftest import golden

NAMES = sorted(dm_oracle.KNOWN)


def _csc(name):
    g = golden(name)
    m, n = int(g["C_mn"][0]), int(g["C_mn"][1])
    p, i = g["C_p"].astype(np.int64), g["C_i"].astype(np.int64)
    return m, n, p, i[:p[n]]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_reproduces_the_reference_known_answers(name):
    m, n, p, i = _csc(name)
    d = dm_oracle.dm(m, n, p, i)
    assert (d["nb"], d["singletons"], d["sprank"]) == dm_oracle.KNOWN[name]


@pytest.mark.parametrize("name", NAMES)
def test_oracle_agrees_with_scipy(name):
    m, n, p, i = _csc(name)
    S = sp.csc_matrix((np.ones(len(i)), i, p), shape=(m, n))
    d = dm_oracle.dm(m, n, p, i)
    assert d["sprank"] == csgraph.structural_rank(S)
    rm, cm = d["rowmatch"], d["colmatch"]
    for j in range(n):             # every matched pair is an entry
        if cm[j] >= 0:
            assert cm[j] in set(i[p[j]:p[j + 1]].tolist()) and rm[cm[j]] == j
    # the fine blocks of A(R2, C2) are the strong components of its graph (column identified with its matched row)
    C2 = sorted(d["C2"])
    if C2:
        rows = [cm[j] for j in C2]
        sub = S[rows][:, C2].tocoo()
        G = sp.csr_matrix((np.ones(sub.nnz), (sub.row, sub.col)), shape=(len(C2), len(C2)))
        ncomp, lab = csgraph.connected_components(G, directed=True, connection="strong")
        fine = set(frozenset(C2[k] for k in np.flatnonzero(lab == c)) for c in range(ncomp))
        assert fine <= set(cs for rs, cs in d["blocks"])
        assert sum(1 for rs, cs in d["blocks"] if cs and cs <= d["C2"]) == ncomp


def test_oracle_on_small_shapes():
    # empty, all-empty columns, wide and tall
    assert dm_oracle.dm(0, 0, [0], [])["nb"] == 0
    d = dm_oracle.dm(3, 2, [0, 0, 0], [])
    assert d["sprank"] == 0 and d["C01"] == {0, 1} and d["R30"] == {0, 1, 2} and d["nb"] == 2
    d = dm_oracle.dm(2, 3, [0, 2, 3, 4], [0, 1, 1, 0])
    assert d["sprank"] == 2 and d["C01"] == {0, 1, 2} and d["nb"] == 1


def test_randperm_conventions():
    import csparse as cs
    assert cs.cs_randperm(5, 0) is None
    assert cs.cs_randperm(5, -1) == [4, 3, 2, 1, 0]
    for seed in (1, 2, 12345, -7):
        p = cs.cs_randperm(1000, seed)
        assert sorted(p) == list(range(1000))
        assert p == cs.cs_randperm(1000, seed)
    assert cs.cs_randperm(1000, 1) != cs.cs_randperm(1000, 2)
    assert cs.cs_randperm(0, 3) == []
    # the documented generator, restated: ascending upper halves of splitmix64(splitmix64(seed) + k)
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9E3779B97F4A7C15) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    sh = mix(3)
    keys = [(mix((sh + k) & M) >> 32, k) for k in range(50)]
    assert cs.cs_randperm(50, 3) == [k for _, k in sorted(keys)]


def test_dalloc_shapes():
    import csparse as cs
    D = cs.cs_dalloc(4, 7)
    assert (len(D.p), len(D.r), len(D.q), len(D.s), len(D.rr), len(D.cc)) == (4, 10, 7, 13, 5, 5)
    assert D.nb == 0
