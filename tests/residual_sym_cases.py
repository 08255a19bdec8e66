"""Inputs shared by the tests of csx_residual_sym_block and of cholsol_factor's refine() -- TEST
INFRASTRUCTURE, NOT PRODUCT.

Storages of one symmetric operator, from any square CSC (n, p, i, x) whose entries with row <= column define it:
  upper_only():    the strictly lower entries dropped, everything else where it was
  with_lower():    upper_only() plus, for every strictly upper entry (r, c), an entry (c, r) in column r -- the mirror's value
                   (a fully stored matrix) or some other value (foreign=True) -- put at random places between the upper
                   entries of its column, which keep their order
  full_sorted():   the fully stored matrix with ascending rows in every column, duplicates in their storage order: the
                   storage on which the symmetric rule and csx_residual_block(trans = 0) take the same terms in the same order

perturbed_spd(seed): the refinement fixture.  About 64 dense SPD blocks of 2 .. 6 rows, each M M' + SHIFT I with M uniform in
(-1, 1), stored as the upper triangle: A, which is factored.  A2 = A o (1 + 1e-6 P), P symmetric and uniform in (-1, 1): the
operator refinement runs against.  A solve with A's factor has a backward error of about 1e-6 against A2; the iteration
x += A^-1 (b - A2 x) contracts by |A^-1 (A2 - A)| <= 1e-6 cond(A) per step, and cond(A) <= (|M|^2 + SHIFT) / SHIFT <= 37 for
a 6 x 6 block with SHIFT = 1, so two steps reach the rounding level from 1e-6."""
import numpy as np

SEEDS = (21, 22, 23)
SHIFT = 1.0
EPS = 2.0 ** -52


def _columns(n, p):
    return np.repeat(np.arange(n, dtype=np.int64), np.diff(np.asarray(p, np.int64)))


def _csc(n, cols, rows, vals):
    """CSC arrays of entries already in column-major storage order"""
    p = np.concatenate([[0], np.cumsum(np.bincount(cols, minlength=n))]).astype(np.int32)
    return n, p, np.asarray(rows, np.int32), np.asarray(vals, np.float64)


def upper_only(n, p, i, x):
    i, x = np.asarray(i, np.int64), np.asarray(x, np.float64)
    cols = _columns(n, p)
    keep = i <= cols
    return _csc(n, cols[keep], i[keep], x[keep])


def with_lower(n, p, i, x, seed, foreign):
    rng = np.random.default_rng(seed)
    n, up, ui, ux = upper_only(n, p, i, x)
    cols = _columns(n, up)
    strict = ui < cols
    lc, lr = ui[strict].astype(np.int64), cols[strict]                          # entry (c, r) goes to column r
    lv = rng.uniform(20.0, 30.0, len(lc)) if foreign else ux[strict]
    allc = np.concatenate([cols, lc])
    allr = np.concatenate([ui.astype(np.int64), lr])
    allv = np.concatenate([ux, lv])
    # upper entries keep their relative order (ascending keys), the lower ones fall between them at random
    key = np.concatenate([np.arange(len(cols), dtype=np.float64), rng.uniform(-1.0, len(cols), len(lc))])
    order = np.lexsort((key, allc))
    return _csc(n, allc[order], allr[order], allv[order])


def full_sorted(n, p, i, x):
    n, up, ui, ux = upper_only(n, p, i, x)
    cols = _columns(n, up)
    pos = np.arange(len(cols))
    strict = ui < cols
    allc = np.concatenate([cols, ui[strict].astype(np.int64)])
    allr = np.concatenate([ui.astype(np.int64), cols[strict]])
    allv = np.concatenate([ux, ux[strict]])
    allq = np.concatenate([pos, pos[strict]])
    order = np.lexsort((allq, allr, allc))
    return _csc(n, allc[order], allr[order], allv[order])


def dense(n, p, i, x):
    """S as a dense array: the entries with row <= column summed and mirrored"""
    S = np.zeros((n, n))
    cols = _columns(n, p)
    for r, c, v in zip(np.asarray(i).tolist(), cols.tolist(), np.asarray(x).tolist()):
        if r <= c:
            S[r, c] += v
            if r < c:
                S[c, r] += v
    return S


def perturbed_spd(seed, nblocks=64):
    """(n, Ap, Ai, Ax, Ax2): the upper triangle of A (sorted columns) and the values of A2 on that pattern"""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(2, 7, nblocks)
    Ap, Ai, Ax, Ax2 = [0], [], [], []
    start = 0
    for s in sizes.tolist():
        M = rng.uniform(-1.0, 1.0, (s, s))
        blk = M @ M.T + SHIFT * np.eye(s)
        P = rng.uniform(-1.0, 1.0, (s, s))
        for j in range(s):
            for r in range(j + 1):
                Ai.append(start + r)
                Ax.append(float(blk[r, j]))
                Ax2.append(float(blk[r, j] * (1.0 + 1e-6 * P[r, j])))
            Ap.append(len(Ai))
        start += s
    return start, np.asarray(Ap, np.int32), np.asarray(Ai, np.int32), np.asarray(Ax), np.asarray(Ax2)


def rhs(n, k, seed):
    return np.random.default_rng(1000 + seed).uniform(-1.0, 1.0, (n, k))


def _phase_lengths():
    """(phase-1 terms, phase-2 terms) of the shaped rows: every pair out of 0, 1, 7, 8 and 9"""
    return [(a, b) for a in (0, 1, 7, 8, 9) for b in (0, 1, 7, 8, 9)]


def edge_matrix(seed=5, n=200):
    """The 200-row matrix of the device tests: rows 40 .. 64 have every pair of phase-1 and phase-2 term counts out of 0, 1, 7,
    8 and 9 (around the 8 entries in flight); rows 100 .. 109 and columns 100 .. 109 are empty; row 70 has no diagonal; the
    columns are unsorted; there are duplicates above, on and below the diagonal, and strictly lower entries with other values."""
    rng = np.random.default_rng(seed)
    ent = []                                                                    # (row, column, value), any order
    empty = set(range(100, 110))
    pairs = _phase_lengths()
    shaped = {40 + t: pr for t, pr in enumerate(pairs)}
    for r, (a, b) in shaped.items():
        # phase 1 of row r: entries (j, r), j <= r, in column r; phase 2: entries (r, j), j > r, in columns j
        below = rng.choice(np.arange(0, 40), a, replace=False)                  # columns 0 .. 39 hold nothing else in these rows
        above = rng.choice(np.arange(120, n), b, replace=False)
        ent += [(int(j), r, float(rng.standard_normal())) for j in below]
        ent += [(r, int(j), float(rng.standard_normal())) for j in above]
    for r in list(range(0, 40)) + list(range(65, 100)) + list(range(110, 120)):
        if r != 70:
            ent.append((r, r, float(rng.uniform(1.0, 2.0))))
        for j in rng.choice(np.arange(65, 100), 3, replace=False).tolist():
            if j > r:
                ent.append((r, j, float(rng.standard_normal())))
    ent += [(66, 66, 0.25), (66, 66, -0.5), (67, 90, 1.5), (67, 90, 2.5)]        # duplicates on and above the diagonal
    ent = [e for e in ent if e[0] not in empty and e[1] not in empty]
    # strictly lower entries: never read as values; duplicates among them too
    low = [(c, r, float(rng.uniform(20.0, 30.0))) for r, c, _ in ent if r < c and rng.random() < 0.5]
    low += [(95, 67, 9.0), (95, 67, 8.0)]
    ent += [e for e in low if e[0] not in empty and e[1] not in empty]
    order = rng.permutation(len(ent))                                           # unsorted columns
    ent = [ent[t] for t in order]
    cols = np.array([e[1] for e in ent], np.int64)
    by_col = np.argsort(cols, kind="stable")
    return _csc(n, cols[by_col], np.array([e[0] for e in ent])[by_col], np.array([e[2] for e in ent])[by_col])
