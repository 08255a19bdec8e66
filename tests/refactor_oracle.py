"""The refactor rule, CPU side -- TEST INFRASTRUCTURE, NOT PRODUCT.

refactor(): new values for the factors of csparse_oracle.cs_lu with its pivots and the patterns of L and U kept.  Column
k of the factorisation, in pivot-row space: x = 0 on the rows of U(:,k) and L(:,k); x[pinv[i]] = A2(i, k) in storage
order (assignment, as cs_spsolve); for every entry J of U(:,k) in storage order but the last (the diagonal): U.x = x[J],
x[L.i[t]] -= L.x[t] * x[J] over L(:,J) after its unit diagonal (multiply and subtract rounded separately); the pivot x[k]
goes last into U(:,k); L.x = x / pivot after the unit diagonal.  Python floats round every operation: whenever cs_lu(A2)
chooses the same pinv, L and U are byte-equal to its own."""
import numpy as np


def _arrays(M):
    n = len(M.p) - 1 if not isinstance(M, tuple) else len(M[0]) - 1
    p, i, x = (M.p, M.i, M.x) if not isinstance(M, tuple) else M
    nnz = int(p[n])
    return [int(v) for v in p], [int(v) for v in i[:nnz]], [float(v) for v in x[:nnz]]


def refactor(L, U, pinv, A2):
    """(Lx, Ux, ok, ratio): L, U, A2 `cs` objects or (p, i, x); A2's column k is column k of the factorisation.
    ok False at the first pivot that is 0 or not finite (then Lx / Ux hold the columns before it).  ratio: min over the
    columns of |pivot| / max |x_i| over L(:,k)'s rows, the pivot included."""
    Lp, Li, Lx = _arrays(L)
    Up, Ui, Ux = _arrays(U)
    Ap, Ai, Ax = _arrays(A2)
    n = len(Lp) - 1
    pinv = [int(v) for v in pinv]
    x = [0.0] * n
    ratio = 1.0
    for k in range(n):
        ue = Up[k + 1] - 1
        for t in range(Up[k], ue + 1):
            x[Ui[t]] = 0.0
        for t in range(Lp[k], Lp[k + 1]):
            x[Li[t]] = 0.0
        for t in range(Ap[k], Ap[k + 1]):
            x[pinv[Ai[t]]] = Ax[t]
        for t in range(Up[k], ue):
            J = Ui[t]
            xj = x[J]
            Ux[t] = xj
            for s in range(Lp[J] + 1, Lp[J + 1]):
                x[Li[s]] = x[Li[s]] - Lx[s] * xj
        piv = x[k]
        Ux[ue] = piv
        big = abs(piv)
        for s in range(Lp[k] + 1, Lp[k + 1]):
            big = max(big, abs(x[Li[s]]))
        if piv == 0.0 or not np.isfinite(piv):
            return Lx, Ux, False, ratio
        ratio = min(ratio, abs(piv) / big)
        Lx[Lp[k]] = 1.0
        for s in range(Lp[k] + 1, Lp[k + 1]):
            Lx[s] = x[Li[s]] / piv
    return Lx, Ux, True, ratio
