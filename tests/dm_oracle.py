"""A small pure-Python Dulmage-Mendelsohn oracle written from the textbook definitions (maximum matching by
augmenting paths, alternating breadth-first searches for the coarse sets, Tarjan for the strongly connected
components of the square part).  It returns only what the decomposition fixes whatever the matching: the coarse
sets, the row and column sets of every fine block, nb and the structural rank."""
from collections import deque

import numpy as np


def _cols(m, n, p, i):
    return [np.unique(np.asarray(i[p[j]:p[j + 1]], dtype=np.int64)).tolist() for j in range(n)]


def matching(m, n, p, i):
    """Maximum matching: (row -> column, column -> row), -1 where unmatched.  Breadth-first augmenting paths."""
    cols = _cols(m, n, p, i)
    rm, cm = [-1] * m, [-1] * n
    for j in range(n):                   # cheap start: the first free row of every column
        for r in cols[j]:
            if rm[r] < 0:
                rm[r], cm[j] = j, r
                break
    for root in range(n):
        if cm[root] >= 0:
            continue
        par = {}                          # row -> column it was reached from
        dq = deque([root])
        end = -1
        while dq and end < 0:
            j = dq.popleft()
            for r in cols[j]:
                if r in par:
                    continue
                par[r] = j
                if rm[r] < 0:
                    end = r
                    break
                dq.append(rm[r])
        while end >= 0:                   # flip the path
            j = par[end]
            nxt = cm[j]
            cm[j], rm[end] = end, j
            end = nxt
    return rm, cm


def _rows(m, n, p, i):
    rows = [[] for _ in range(m)]
    for j in range(n):
        for r in set(i[p[j]:p[j + 1]]):
            rows[int(r)].append(j)
    return rows


def tarjan(nv, succ):
    """Strongly connected components (iterative Tarjan); a list of vertex lists."""
    index, low, on, st, out = [-1] * nv, [0] * nv, [False] * nv, [], []
    counter = 0
    for s in range(nv):
        if index[s] >= 0:
            continue
        work = [(s, 0)]
        index[s] = low[s] = counter
        counter += 1
        st.append(s)
        on[s] = True
        while work:
            v, k = work[-1]
            if k < len(succ[v]):
                work[-1] = (v, k + 1)
                w = succ[v][k]
                if index[w] < 0:
                    index[w] = low[w] = counter
                    counter += 1
                    st.append(w)
                    on[w] = True
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    u = work[-1][0]
                    low[u] = min(low[u], low[v])
                if low[v] == index[v]:
                    comp = []
                    while True:
                        w = st.pop()
                        on[w] = False
                        comp.append(w)
                        if w == v:
                            break
                    out.append(comp)
    return out


def dm(m, n, p, i):
    """Canonical parts of the DM decomposition of the m x n pattern (p, i):
    dict(sprank, nb, singletons, C01, C2, C3, R1, R2, R30, blocks) -- sets as frozensets, blocks a set of
    (frozenset rows, frozenset cols) pairs of every fine block."""
    p = [int(v) for v in p]
    i = [int(v) for v in i[:p[n]]] if n else []
    rm, cm = matching(m, n, p, i)
    cols, rows = _cols(m, n, p, i), _rows(m, n, p, i)
    # columns reachable from unmatched columns along alternating paths; the rows they touch
    C01, R1 = set(j for j in range(n) if cm[j] < 0), set()
    dq = deque(C01)
    while dq:
        j = dq.popleft()
        for r in cols[j]:
            if r in R1:
                continue
            R1.add(r)
            j2 = rm[r]
            if j2 >= 0 and j2 not in C01:
                C01.add(j2)
                dq.append(j2)
    # rows reachable from unmatched rows; the columns they touch
    R30, C3 = set(r for r in range(m) if rm[r] < 0), set()
    dq = deque(R30)
    while dq:
        r = dq.popleft()
        for j in rows[r]:
            if j in C3 or j in C01:
                continue
            C3.add(j)
            r2 = cm[j]
            if r2 >= 0 and r2 not in R30:
                R30.add(r2)
                dq.append(r2)
    C2 = [j for j in range(n) if j not in C01 and j not in C3]
    R2 = [cm[j] for j in C2]
    sprank = sum(1 for j in range(n) if cm[j] >= 0)
    vert = {j: k for k, j in enumerate(C2)}
    succ = [[] for _ in C2]            # entry (row matched to column u, column w) is the edge u -> w
    for k, j in enumerate(C2):
        for w in rows[cm[j]]:
            if w in vert and vert[w] != k:
                succ[k].append(vert[w])
    blocks = []
    if C01:
        blocks.append((frozenset(R1), frozenset(C01)))
    for comp in tarjan(len(C2), succ):
        blocks.append((frozenset(cm[C2[v]] for v in comp), frozenset(C2[v] for v in comp)))
    if R30:
        blocks.append((frozenset(R30), frozenset(C3)))
    nb = len(blocks)
    singletons = sum(1 for rs, cs in blocks if len(rs) == 1 and len(cs) == 1)
    blocks = set(blocks)
    return dict(sprank=sprank, nb=nb, singletons=singletons, C01=frozenset(C01), C2=frozenset(C2), C3=frozenset(C3),
                R1=frozenset(R1), R2=frozenset(R2), R30=frozenset(R30), blocks=blocks, rowmatch=rm, colmatch=cm)


# The reference test file's known answers (csparse_test.py Test2): (nb, singletons, structural rank)
KNOWN = {
    "ash219": (1, 0, 85), "bcsstk01": (1, 0, 48), "bcsstk16": (75, 74, 4884), "fs_183_1": (38, 37, 183),
    "ibm32a": (1, 0, 31), "ibm32b": (1, 0, 31), "lp_afiro": (1, 0, 27), "mbeacxc": (10, 8, 448), "t1": (1, 0, 4),
    "west0067": (2, 1, 67),
}
