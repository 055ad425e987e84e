/* ORACLE (test infrastructure only). Included by seq_adjoint.c once per arithmetic type REAL (long double: the reference;
 * double: only to show how much rounding the long-double build removes); every name is suffixed through RNAME().
 *
 * The reverse-mode derivative of the FULL sequential recursion of seq_kalman_body.inc (seq_filter: predict, scalar update,
 * the per-step log term; time-varying covariance, no stationarity assumption) with respect to the shared blocks A, a, Q, H, h, R
 * and x0m, x0P. Run-time state dimension d <= ADJ_MAXD (64: the wide-state engine's models too); column-major d x d blocks as in
 * seq_kalman_body.inc. The d x d work arrays live on the heap beside the kept steps (eleven of them: 0.7 MB in long double at d = 64, and the
 * oracle may be called off the main thread); only d-vectors are on the stack.
 *
 * Forward, step t (m, P: the filtered state of step t - 1; x0m, x0P before the first), as seq_kalman_body.inc / lgssm_ref.py:
 *     S  = Symmetric(P)  (upper triangle mirrored)      mp = A m + a         Pp = A S A' + Q
 *     V  = Pp' H         s = V . H + R                  e  = y_t - (H . mp + h)
 *     m  = mp + V e / s  P = Pp - V V' / s              l_t = -(log 2 pi + log s + e^2 / s) / 2
 * The forward pass keeps mp and Pp of every step, T (d^2 + d) values; V, s, e and the filtered state of step t - 1 are
 * recomputed from them on the way back. Backward, step t (mb, Pb: the adjoints of the filtered m, P of step t; zero behind the
 * last step; the adjoint of every l_t is 1):
 *     l_t:           sb = -(1 / s - e^2 / s^2) / 2          eb = -e / s
 *     m:             mpb = mb     Vb = mb e / s             eb += (mb . V) / s      sb -= (mb . V) e / s^2
 *     P:             Ppb = Pb     Vb -= (Pb + Pb') V / s    sb += (V' Pb V) / s^2
 *     e:             Hb -= eb mp  mpb -= eb H               hb -= eb
 *     s:             Vb += sb H   Hb += sb V                Rb += sb
 *     V = Pp' H:     Hb += Pp Vb  Ppb += H Vb'
 *     Pp:            Qb += Ppb    Ab += Ppb A S' + Ppb' A S                         Sb = A' Ppb A
 *     mp:            Ab += mpb m' ab += mpb                 mb <- A' mpb
 *     S:             Pb <- the upper triangle of Sb + Sb' (the diagonal of Sb once), zero below the diagonal
 * and x0mb = mb, x0Pb = Pb in front of the first step. Qb and x0Pb are symmetrised on return (pair them with symmetric tangents).
 */

static int RNAME(seq_adjoint)(int d, int64_t T, const double *A_, const double *a_, const double *Q_, const double *H_, double h_, double R_,
                              const double *y, const double *x0m_, const double *x0P_, double *lml_out, double *gA, double *ga, double *gQ,
                              double *gH, double *gh, double *gR, double *gx0m, double *gx0P) {
    if (d < 1 || d > ADJ_MAXD || T < 1) return 1;
    const int dd = d * d;
    REAL a[ADJ_MAXD], H[ADJ_MAXD], m[ADJ_MAXD], V[ADJ_MAXD];
    const REAL h = (REAL)h_, R = (REAL)R_;
    /* one block: mp and Pp of every step, then the eleven d x d work arrays */
    REAL *mps = (REAL *)malloc(((size_t)T * (size_t)(dd + d) + (size_t)11 * dd) * sizeof(REAL));
    if (!mps) return 3;
    REAL *Pps = mps + (size_t)T * d;
    REAL *A = Pps + (size_t)T * dd, *Q = A + dd, *P = Q + dd, *S = P + dd, *AS = S + dd;
    REAL *Ab = AS + dd, *Qb = Ab + dd, *Pb = Qb + dd, *Ppb = Pb + dd, *X = Ppb + dd, *Sb = X + dd;
    for (int i = 0; i < dd; ++i) { A[i] = (REAL)A_[i]; Q[i] = (REAL)Q_[i]; P[i] = (REAL)x0P_[i]; }
    for (int i = 0; i < d; ++i) { a[i] = (REAL)a_[i]; H[i] = (REAL)H_[i]; m[i] = (REAL)x0m_[i]; }
    REAL acc = 0;
    /* ---- forward */
    for (int64_t t = 0; t < T; ++t) {
        REAL *mp = mps + (size_t)t * d, *Pp = Pps + (size_t)t * dd;
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) S[i + j * d] = (i <= j) ? P[i + j * d] : P[j + i * d];
        for (int i = 0; i < d; ++i) {
            REAL v = 0;
            for (int k = 0; k < d; ++k) v += A[i + k * d] * m[k];
            mp[i] = v + a[i];
        }
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) {
                REAL v = 0;
                for (int k = 0; k < d; ++k) v += A[i + k * d] * S[k + j * d];
                AS[i + j * d] = v;
            }
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) {
                REAL v = 0;
                for (int k = 0; k < d; ++k) v += AS[i + k * d] * A[j + k * d];
                Pp[i + j * d] = v + Q[i + j * d];
            }
        REAL s = R, hm = 0;
        for (int j = 0; j < d; ++j) {
            REAL v = 0;
            for (int k = 0; k < d; ++k) v += H[k] * Pp[k + j * d];
            V[j] = v;
        }
        for (int k = 0; k < d; ++k) { s += V[k] * H[k]; hm += H[k] * mp[k]; }
        if (!(s > 0)) { free(mps); return 2; }
        const REAL e = (REAL)y[t] - (hm + h);
        for (int i = 0; i < d; ++i) m[i] = mp[i] + V[i] * e / s;
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) P[i + j * d] = Pp[i + j * d] - V[i] * V[j] / s;
        acc += -((REAL)LOG2PI_L + RLOG(s) + e * e / s) / 2;
    }
    /* ---- backward */
    REAL ab[ADJ_MAXD], Hb[ADJ_MAXD], hb = 0, Rb = 0, mb[ADJ_MAXD];
    for (int i = 0; i < dd; ++i) { Ab[i] = 0; Qb[i] = 0; Pb[i] = 0; }
    for (int i = 0; i < d; ++i) { ab[i] = 0; Hb[i] = 0; mb[i] = 0; }
    for (int64_t t = T - 1; t >= 0; --t) {
        const REAL *mp = mps + (size_t)t * d, *Pp = Pps + (size_t)t * dd;
        REAL s = R, hm = 0;
        for (int j = 0; j < d; ++j) {
            REAL v = 0;
            for (int k = 0; k < d; ++k) v += H[k] * Pp[k + j * d];
            V[j] = v;
        }
        for (int k = 0; k < d; ++k) { s += V[k] * H[k]; hm += H[k] * mp[k]; }
        const REAL e = (REAL)y[t] - (hm + h);
        /* the filtered state of step t - 1 (what this step's predict read) */
        if (t == 0) {
            for (int i = 0; i < dd; ++i) P[i] = (REAL)x0P_[i];
            for (int i = 0; i < d; ++i) m[i] = (REAL)x0m_[i];
        } else {
            const REAL *mq = mps + (size_t)(t - 1) * d, *Pq = Pps + (size_t)(t - 1) * dd;
            REAL Vq[ADJ_MAXD], sq = R, hq = 0;
            for (int j = 0; j < d; ++j) {
                REAL v = 0;
                for (int k = 0; k < d; ++k) v += H[k] * Pq[k + j * d];
                Vq[j] = v;
            }
            for (int k = 0; k < d; ++k) { sq += Vq[k] * H[k]; hq += H[k] * mq[k]; }
            const REAL eq = (REAL)y[t - 1] - (hq + h);
            for (int i = 0; i < d; ++i) m[i] = mq[i] + Vq[i] * eq / sq;
            for (int j = 0; j < d; ++j)
                for (int i = 0; i < d; ++i) P[i + j * d] = Pq[i + j * d] - Vq[i] * Vq[j] / sq;
        }
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) S[i + j * d] = (i <= j) ? P[i + j * d] : P[j + i * d];
        REAL mbV = 0, VPV = 0, Vb[ADJ_MAXD], mpb[ADJ_MAXD];
        for (int i = 0; i < d; ++i) mbV += mb[i] * V[i];
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) VPV += V[i] * Pb[i + j * d] * V[j];
        REAL sb = -(1 / s - e * e / (s * s)) / 2 - mbV * e / (s * s) + VPV / (s * s);
        REAL eb = -e / s + mbV / s;
        for (int i = 0; i < d; ++i) {
            REAL v = 0;
            for (int j = 0; j < d; ++j) v += (Pb[i + j * d] + Pb[j + i * d]) * V[j];
            Vb[i] = mb[i] * e / s - v / s + sb * H[i];
            mpb[i] = mb[i] - eb * H[i];
        }
        for (int i = 0; i < dd; ++i) Ppb[i] = Pb[i];
        hb -= eb;
        Rb += sb;
        for (int k = 0; k < d; ++k) {
            REAL v = 0;
            for (int j = 0; j < d; ++j) v += Pp[k + j * d] * Vb[j];
            Hb[k] += -eb * mp[k] + sb * V[k] + v;
            for (int j = 0; j < d; ++j) Ppb[k + j * d] += H[k] * Vb[j];
        }
        /* Pp = A S A' + Q */
        for (int i = 0; i < dd; ++i) Qb[i] += Ppb[i];
        for (int j = 0; j < d; ++j)              /* AS = A S (S symmetric) */
            for (int i = 0; i < d; ++i) {
                REAL v = 0;
                for (int k = 0; k < d; ++k) v += A[i + k * d] * S[k + j * d];
                AS[i + j * d] = v;
            }
        for (int j = 0; j < d; ++j)              /* Ab += (Ppb + Ppb') A S + mpb m' */
            for (int i = 0; i < d; ++i) {
                REAL v = 0;
                for (int k = 0; k < d; ++k) v += (Ppb[i + k * d] + Ppb[k + i * d]) * AS[k + j * d];
                Ab[i + j * d] += v + mpb[i] * m[j];
            }
        for (int j = 0; j < d; ++j)              /* X = Ppb A */
            for (int i = 0; i < d; ++i) {
                REAL v = 0;
                for (int k = 0; k < d; ++k) v += Ppb[i + k * d] * A[k + j * d];
                X[i + j * d] = v;
            }
        for (int j = 0; j < d; ++j)              /* Sb = A' X */
            for (int i = 0; i < d; ++i) {
                REAL v = 0;
                for (int k = 0; k < d; ++k) v += A[k + i * d] * X[k + j * d];
                Sb[i + j * d] = v;
            }
        for (int i = 0; i < d; ++i) ab[i] += mpb[i];
        for (int i = 0; i < d; ++i) {
            REAL v = 0;
            for (int k = 0; k < d; ++k) v += A[k + i * d] * mpb[k];
            mb[i] = v;
        }
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) Pb[i + j * d] = (i < j) ? Sb[i + j * d] + Sb[j + i * d] : (i == j ? Sb[i + j * d] : 0);
    }
    *lml_out = (double)acc;
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) {
            gA[i + j * d] = (double)Ab[i + j * d];
            gQ[i + j * d] = (double)((Qb[i + j * d] + Qb[j + i * d]) / 2);
            gx0P[i + j * d] = (double)((Pb[i + j * d] + Pb[j + i * d]) / 2);
        }
    for (int i = 0; i < d; ++i) { ga[i] = (double)ab[i]; gH[i] = (double)Hb[i]; gx0m[i] = (double)mb[i]; }
    *gh = (double)hb;
    *gR = (double)Rb;
    free(mps);      /* (behind the copies: Ab, Qb and Pb live in it) */
    return 0;
}
