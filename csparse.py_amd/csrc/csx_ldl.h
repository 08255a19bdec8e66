// The one partial-LDL' factor object with its build, run and refactor (csx_ldl.hip), on which csx_ldl_factor (n1 = n: nothing
// kept) and csx_schur_factor (csx_schur.hip) both stand.  The level walk under it is csx_levelwalk.h's.
#pragma once
#include "csx_colupdate.h"
#include "csx_levelwalk.h"

namespace csx {

constexpr int LDL_ACC = 512;    // column entries kept in LDS per wave (24 KB a workgroup); longer columns are updated in place in global memory

// The partial LDL' of P A P' = Lp blockdiag(D1, S) Lp': the first n1 columns eliminated, the Schur complement S of the last
// ns = n - n1 left.  n1 == n is the LDL' factor itself: no trailing column, no chunk, an empty S, and Lp's pattern IS the full
// pattern.  Handles of both kinds (K_LDLFACTOR, K_SCHURFACTOR) own one of these.
struct LdlFactor : LevelFactor {            // (the levels are those of the first n1 columns)
    int32_t n1 = 0, ns = 0, lnz = 0, head = 0;   // lnz: entries of the full pattern of chol(P A P'); head = its p[n1]
    const int32_t *Lp = nullptr, *Li = nullptr;   // the full pattern the kernels read: the committed L's own p / i for ns == 0, ...
    DevBuf<int32_t> fp, fi;                 // ... these for ns > 0 (L then holds the interior columns and a unit tail)
    DevBuf<int32_t> rp, rc, rpos;           // row view of the full pattern (chol_symbolic_device)
    DevBuf<int32_t> win;                    // the entry map
    DevBuf<int32_t> ch_col, ch_row0;        // csx_schur.hip: the (column, first row) pairs of the trailing-column kernel
    int64_t chunks = 0;
    csx_handle_t hL = 0, hd = 0, hS = 0;    // the committed Lp, d, S: owned here, lent out by csx_ldl_parts / csx_schur_parts
    DevBuf<double> Lx, dd, Sx;              // scratch of a run: committed only when none of the n1 columns broke down
    // flags: [1] perturbed pivots, [2] columns updated in place; stats: k_ldl_stats' five words
    // csx_ldl_info / csx_schur_info, csx_ldl_stats / csx_schur_stats
    int64_t schur_launches = 0, pos = 0, neg = 0, perturbed = 0;
    double min_d = 0.0, max_d = 0.0, max_l = 0.0;
    ~LdlFactor() {
        if (hL) (void)csx_free(hL);
        if (hd) (void)csx_free(hd);
        if (hS) (void)csx_free(hS);
    }
};

// csx_ldl.hip.  ldl_build: the analysis of A under the caller's S (host parent, cp, pinv) for the elimination of the first n1
// columns, the walker taking at most run_levels levels a launch, and the committed parts allocated.  ldl_run: the factor of the
// values Ax (A's storage order) into the scratch arrays, with the statistics of what was computed; Lp.x, d and S are committed
// when none of the n1 columns broke down.  *ok: 1 committed, 0 breakdown (nothing touched).  Synchronises.  ldl_refactor: ldl_run on the values of A2 after the pattern check
// (*ok = -1, CSX_EINVAL: not A's pattern or length); F null (a handle of another kind) is CSX_EINVAL with *ok untouched.
int ldl_build(Csc *A, const int32_t *parent, const int32_t *cp, const int32_t *pinv, int32_t n1, int32_t run_levels, const char *who,
              LdlFactor *F);
int ldl_run(LdlFactor *F, const double *Ax, double tau, int *ok);
int ldl_refactor(LdlFactor *F, csx_handle_t hA2, double tau, int *ok);
int ldl_stats(const LdlFactor *F, double *out);   // min |d|, max |d|, max |l| of the committed factor
// csx_schur.hip: k_schur_cols over F's chunks -- S into F->Sx from the finished first n1 columns in F->Lx / F->dd -- queued on
// the context's stream
void schur_launch_cols(const LdlFactor *F);

}  // namespace csx
