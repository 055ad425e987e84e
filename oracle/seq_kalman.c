/* ORACLE (test infrastructure only -- never linked into the product library).
 * C restatement of the reference's sequential scalar-output Kalman recursions with compile-time
 * state dimension for d <= 8 (the analogue of the reference's SArrayStorage path: fully unrolled fixed-size
 * stack matrices), and with a run-time state dimension for 8 < d <= 64 (the same recursions on heap
 * buffers, loops ordered for the vectoriser: the checker of the wide-state engine at lengths the NumPy
 * restatement cannot finish). Used (a) as the large-T checker for the HIP path and (b) by bench.py's
 * `cpu_baseline` leg (kind "port", 1 core -- the reference's scan is single-threaded,
 * /root/reference/src/util/scan.jl:15-28). See seq_kalman_body.inc for the per-function citations.
 * PARITY UNPINNED vs reference-run outputs (no Julia in this image); checked against
 * oracle/lgssm_ref.py (tests/test_oracle_c.py), which the reference's identities pin.
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define LOG2PI 1.8378770664093454835606594728112
#define CAT_(a, b) a##_d##b
#define CAT(a, b) CAT_(a, b)
#define NAME(f) CAT(f, D)

#define D 1
#include "seq_kalman_body.inc"
#undef D
#define D 2
#include "seq_kalman_body.inc"
#undef D
#define D 3
#include "seq_kalman_body.inc"
#undef D
#define D 4
#include "seq_kalman_body.inc"
#undef D
#define D 5
#include "seq_kalman_body.inc"
#undef D
#define D 6
#include "seq_kalman_body.inc"
#undef D
#define D 7
#include "seq_kalman_body.inc"
#undef D
#define D 8
#include "seq_kalman_body.inc"
#undef D

/* ------------------------------------------------------------------------------------------------
 * Run-time state dimension (8 < d <= DYN_MAX). The same steps as seq_kalman_body.inc, statement by
 * statement and with every sum in the same order (k ascending), on heap buffers; the matrix products
 * run their innermost loop down a column so that the compiler vectorises them. Return code 3: out of
 * memory. seq_posterior_marginals_dyn keeps the filtered state every `blk` steps only and rebuilds the
 * reverse dynamics of one block at a time from it (the same numbers as one pass storing all of them:
 * the filter restarted from a stored state repeats its steps bit for bit), so that series of several
 * million steps fit in memory; its caller-provided G, g, L are not used and may be NULL. */
#define DYN_MAX 64

static void dyn_sym_upper(int d, const double *P, double *S) {
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) S[i + j * d] = (i <= j) ? P[i + j * d] : P[j + i * d];
}

/* C = X * Y (tY == 0) or X * Y' (tY == 1), all d x d column-major; C must not alias X or Y */
static void dyn_mul(int d, const double *X, const double *Y, int tY, double *C) {
    for (int j = 0; j < d; ++j) {
        double *restrict c = C + j * d;
        for (int i = 0; i < d; ++i) c[i] = 0.0;
        for (int k = 0; k < d; ++k) {
            const double y = tY ? Y[j + k * d] : Y[k + j * d];
            const double *restrict x = X + k * d;
            for (int i = 0; i < d; ++i) c[i] += x[i] * y;
        }
    }
}

/* w: 2 d^2 + d doubles */
static void dyn_predict(int d, const double *A, const double *a, const double *Q, double *m, double *P, double *w) {
    double *S = w, *AS = w + d * d, *mp = w + 2 * d * d;
    dyn_sym_upper(d, P, S);
    for (int i = 0; i < d; ++i) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc += A[i + k * d] * m[k];
        mp[i] = acc + a[i];
    }
    dyn_mul(d, A, S, 0, AS);
    dyn_mul(d, AS, A, 1, P);
    for (int i = 0; i < d * d; ++i) P[i] += Q[i];
    for (int i = 0; i < d; ++i) m[i] = mp[i];
}

/* w: 2 d doubles */
static double dyn_update(int d, const double *H, double h, double R, double y, double *m, double *P, double *w) {
    double *V = w, *B = w + d;
    for (int j = 0; j < d; ++j) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc += H[k] * P[k + j * d];
        V[j] = acc;
    }
    double s2 = 0.0, hm = 0.0;
    for (int k = 0; k < d; ++k) { s2 += V[k] * H[k]; hm += H[k] * m[k]; }
    double sqrtS = sqrt(s2 + R);
    for (int j = 0; j < d; ++j) B[j] = V[j] / sqrtS;
    double alpha = (y - (hm + h)) / sqrtS;
    for (int i = 0; i < d; ++i) m[i] += B[i] * alpha;
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) P[i + j * d] -= B[i] * B[j];
    return -(LOG2PI + 2.0 * log(sqrtS) + alpha * alpha) / 2.0;
}

static int dyn_chol_upper(int d, const double *S, double *U) {
    for (int j = 0; j < d; ++j) {
        for (int i = 0; i <= j; ++i) {
            double acc = S[i + j * d];
            for (int k = 0; k < i; ++k) acc -= U[k + i * d] * U[k + j * d];
            if (i == j) {
                if (!(acc > 0.0)) return 1;
                U[j + j * d] = sqrt(acc);
            } else {
                U[i + j * d] = acc / U[i + i * d];
            }
        }
        for (int i = j + 1; i < d; ++i) U[i + j * d] = 0.0;
    }
    return 0;
}

/* w: 5 d^2 doubles */
static int dyn_invert_dynamics(int d, const double *mf, const double *Pf, const double *mp, const double *Pp,
                               const double *A, double *G, double *g, double *L, double *w) {
    double *Pj = w, *U = w + d * d, *X = w + 2 * d * d, *Gt = w + 3 * d * d, *UG = w + 4 * d * d;
    for (int i = 0; i < d * d; ++i) Pj[i] = Pp[i];
    for (int i = 0; i < d; ++i) Pj[i + i * d] += 1e-10;
    if (dyn_chol_upper(d, Pj, U)) return 1;
    dyn_mul(d, A, Pf, 0, X);
    for (int j = 0; j < d; ++j) {
        for (int i = 0; i < d; ++i) {
            double acc = X[i + j * d];
            for (int k = 0; k < i; ++k) acc -= U[k + i * d] * Gt[k + j * d];
            Gt[i + j * d] = acc / U[i + i * d];
        }
        for (int i = d - 1; i >= 0; --i) {
            double acc = Gt[i + j * d];
            for (int k = i + 1; k < d; ++k) acc -= U[i + k * d] * Gt[k + j * d];
            Gt[i + j * d] = acc / U[i + i * d];
        }
    }
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) G[i + j * d] = Gt[j + i * d];
    for (int i = 0; i < d; ++i) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc += G[i + k * d] * mp[k];
        g[i] = mf[i] - acc;
    }
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) {
            double acc = 0.0;
            for (int k = i; k < d; ++k) acc += U[i + k * d] * Gt[k + j * d];
            UG[i + j * d] = acc;
        }
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) {
            double acc = 0.0;
            for (int k = 0; k < d; ++k) acc += UG[k + i * d] * UG[k + j * d];
            L[i + j * d] = Pf[i + j * d] - acc;
        }
    return 0;
}

/* emission mean / variance of the state (m, P); w: d^2 doubles */
static void dyn_emit(int d, const double *Ht, double h, double R, const double *m, const double *P, double *w,
                     double *mean, double *var) {
    dyn_sym_upper(d, P, w);
    double mu = h, v = R;
    for (int j = 0; j < d; ++j) {
        double acc = 0.0;
        for (int k = 0; k < d; ++k) acc += Ht[k] * w[k + j * d];
        v += acc * Ht[j];
        mu += Ht[j] * m[j];
    }
    *mean = mu; *var = v;
}

#define DYN_WORK(d) ((size_t)(8 * (d) * (d) + 8 * (d)))

static int seq_filter_dyn(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                          const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h, int64_t sh,
                          const double *R, int64_t sR, const double *y, const double *x0m, const double *x0P,
                          double *lml_out, double *m_out, double *P_out) {
    const size_t dd = (size_t)d * d;
    double *buf = malloc((DYN_WORK(d) + dd + d) * sizeof(double));
    if (!buf) return 3;
    double *w = buf, *P = buf + DYN_WORK(d), *m = P + dd, acc = 0.0;
    memcpy(m, x0m, d * sizeof(double)); memcpy(P, x0P, dd * sizeof(double));
    for (int64_t t = 0; t < T; ++t) {
        dyn_predict(d, A + t * sA, a + t * sa, Q + t * sQ, m, P, w);
        acc += dyn_update(d, H + t * sH, h[t * sh], R[t * sR], y[t], m, P, w);
        if (m_out) memcpy(m_out + t * d, m, d * sizeof(double));
        if (P_out) memcpy(P_out + t * dd, P, dd * sizeof(double));
    }
    if (lml_out) *lml_out = acc;
    free(buf);
    return 0;
}

/* steps t0 .. t1 - 1 of the posterior pass from the state (m, P) before step t0; G, g, L indexed from t0 */
static int dyn_posterior_steps(int d, int64_t t0, int64_t t1, const double *A, int64_t sA, const double *a, int64_t sa,
                               const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h, int64_t sh,
                               const double *R, int64_t sR, const double *y, double *m, double *P,
                               double *G, double *g, double *L, double *w) {
    const size_t dd = (size_t)d * d;
    double *Pp = w, *mp = w + dd, *w2 = w + dd + d;
    for (int64_t t = t0; t < t1; ++t) {
        memcpy(mp, m, d * sizeof(double)); memcpy(Pp, P, dd * sizeof(double));
        dyn_predict(d, A + t * sA, a + t * sa, Q + t * sQ, mp, Pp, w2);
        if (dyn_invert_dynamics(d, m, P, mp, Pp, A + t * sA, G + (t - t0) * dd, g + (t - t0) * d, L + (t - t0) * dd, w2)) return 2;
        dyn_update(d, H + t * sH, h[t * sh], R[t * sR], y[t], mp, Pp, w2);
        memcpy(m, mp, d * sizeof(double)); memcpy(P, Pp, dd * sizeof(double));
    }
    return 0;
}

static int seq_posterior_dyn(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                             const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h, int64_t sh,
                             const double *R, int64_t sR, const double *y, const double *x0m, const double *x0P,
                             double *G, double *g, double *L, double *xfm, double *xfP) {
    const size_t dd = (size_t)d * d;
    double *w = malloc(DYN_WORK(d) * sizeof(double));
    if (!w) return 3;
    memcpy(xfm, x0m, d * sizeof(double)); memcpy(xfP, x0P, dd * sizeof(double));
    int rc = dyn_posterior_steps(d, 0, T, A, sA, a, sa, Q, sQ, H, sH, h, sh, R, sR, y, xfm, xfP, G, g, L, w);
    free(w);
    return rc;
}

static int seq_posterior_marginals_dyn(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                                       const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h,
                                       int64_t sh, const double *R, int64_t sR, const double *y,
                                       const double *x0m, const double *x0P, const double *Rnew, int64_t sRn,
                                       double *G_unused, double *g_unused, double *L_unused, double *mean_out, double *var_out) {
    (void)G_unused; (void)g_unused; (void)L_unused;
    const size_t dd = (size_t)d * d, per = 2 * dd + d;
    int64_t blk = (int64_t)((size_t)(1 << 23) / per);      /* 64 MiB of reverse dynamics at a time */
    if (blk < 16) blk = 16;
    if (blk > T) blk = T > 0 ? T : 1;
    const int64_t nblk = (T + blk - 1) / blk;
    double *buf = malloc((DYN_WORK(d) + 2 * (dd + d) + (size_t)blk * per + (size_t)nblk * (dd + d)) * sizeof(double));
    if (!buf) return 3;
    double *w = buf, *P = w + DYN_WORK(d), *m = P + dd, *Pb = m + d, *mb = Pb + dd;
    double *G = mb + d, *L = G + (size_t)blk * dd, *g = L + (size_t)blk * dd, *ck = g + (size_t)blk * d;
    int rc = 0;
    memcpy(m, x0m, d * sizeof(double)); memcpy(P, x0P, dd * sizeof(double));
    for (int64_t t = 0; t < T; ++t) {      /* the filter alone, keeping the state in front of every block */
        if (t % blk == 0) {
            memcpy(ck + (t / blk) * (dd + d), P, dd * sizeof(double));
            memcpy(ck + (t / blk) * (dd + d) + dd, m, d * sizeof(double));
        }
        dyn_predict(d, A + t * sA, a + t * sa, Q + t * sQ, m, P, w);
        dyn_update(d, H + t * sH, h[t * sh], R[t * sR], y[t], m, P, w);
    }
    for (int64_t b = nblk - 1; b >= 0 && !rc; --b) {      /* (m, P): the smoothed state at the block's last step */
        const int64_t t0 = b * blk, t1 = t0 + blk < T ? t0 + blk : T;
        memcpy(Pb, ck + b * (dd + d), dd * sizeof(double));
        memcpy(mb, ck + b * (dd + d) + dd, d * sizeof(double));
        rc = dyn_posterior_steps(d, t0, t1, A, sA, a, sa, Q, sQ, H, sH, h, sh, R, sR, y, mb, Pb, G, g, L, w);
        if (rc) break;
        for (int64_t t = t1 - 1; t >= t0; --t) {
            dyn_emit(d, H + t * sH, h[t * sh], Rnew[t * sRn], m, P, w, mean_out + t, var_out + t);
            dyn_predict(d, G + (t - t0) * dd, g + (t - t0) * d, L + (t - t0) * dd, m, P, w);
        }
    }
    free(buf);
    return rc;
}

static int seq_prior_marginals_dyn(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                                   const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h,
                                   int64_t sh, const double *R, int64_t sR, const double *x0m, const double *x0P,
                                   double *mean_out, double *var_out) {
    const size_t dd = (size_t)d * d;
    double *buf = malloc((DYN_WORK(d) + dd + d) * sizeof(double));
    if (!buf) return 3;
    double *w = buf, *P = buf + DYN_WORK(d), *m = P + dd;
    memcpy(m, x0m, d * sizeof(double)); memcpy(P, x0P, dd * sizeof(double));
    for (int64_t t = 0; t < T; ++t) {
        dyn_predict(d, A + t * sA, a + t * sa, Q + t * sQ, m, P, w);
        dyn_emit(d, H + t * sH, h[t * sh], R[t * sR], m, P, w, mean_out + t, var_out + t);
    }
    free(buf);
    return 0;
}

static int seq_rand_dyn(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                        const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h, int64_t sh,
                        const double *R, int64_t sR, const double *x0m, const double *x0P,
                        const double *eps_t, const double *eps_e, const double *eps_0, double *y_out) {
    const size_t dd = (size_t)d * d;
    double *buf = malloc((2 * dd + 2 * d) * sizeof(double));
    if (!buf) return 3;
    double *Pj = buf, *U = Pj + dd, *x = U + dd, *xn = x + d;
    int rc = 0;
    for (size_t i = 0; i < dd; ++i) Pj[i] = x0P[i];
    for (int i = 0; i < d; ++i) Pj[i + i * d] += 1e-12;
    if (dyn_chol_upper(d, Pj, U)) { free(buf); return 2; }
    for (int i = 0; i < d; ++i) {
        double acc = x0m[i];
        for (int k = 0; k <= i; ++k) acc += U[k + i * d] * eps_0[k];
        x[i] = acc;
    }
    for (int64_t t = 0; t < T; ++t) {
        const double *At = A + t * sA, *Qt = Q + t * sQ, *Ht = H + t * sH, *e = eps_t + t * d;
        if (t == 0 || sQ != 0) {      /* (a shared Q: the same factor at every step) */
            for (size_t i = 0; i < dd; ++i) Pj[i] = Qt[i];
            for (int i = 0; i < d; ++i) Pj[i + i * d] += 1e-9;
            if (dyn_chol_upper(d, Pj, U)) { rc = 2; break; }
        }
        for (int i = 0; i < d; ++i) {
            double acc = a[t * sa + i];
            for (int k = 0; k < d; ++k) acc += At[i + k * d] * x[k];
            double nz = 0.0;
            for (int k = 0; k <= i; ++k) nz += U[k + i * d] * e[k];
            xn[i] = acc + nz;
        }
        double yy = h[t * sh];
        for (int i = 0; i < d; ++i) { x[i] = xn[i]; yy += Ht[i] * xn[i]; }
        y_out[t] = yy + sqrt(R[t * sR]) * eps_e[t];
    }
    free(buf);
    return rc;
}

#define DISPATCH(fn, ...)                                   \
    switch (d) {                                            \
        case 1: return fn##_d1(__VA_ARGS__);                \
        case 2: return fn##_d2(__VA_ARGS__);                \
        case 3: return fn##_d3(__VA_ARGS__);                \
        case 4: return fn##_d4(__VA_ARGS__);                \
        case 5: return fn##_d5(__VA_ARGS__);                \
        case 6: return fn##_d6(__VA_ARGS__);                \
        case 7: return fn##_d7(__VA_ARGS__);                \
        case 8: return fn##_d8(__VA_ARGS__);                \
        default:                                            \
            if (d > 8 && d <= DYN_MAX) return fn##_dyn(d, __VA_ARGS__); \
            return 4;                                       \
    }

int oracle_seq_filter(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                      const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h, int64_t sh,
                      const double *R, int64_t sR, const double *y, const double *x0m, const double *x0P,
                      double *lml_out, double *m_out, double *P_out) {
    DISPATCH(seq_filter, T, A, sA, a, sa, Q, sQ, H, sH, h, sh, R, sR, y, x0m, x0P, lml_out, m_out, P_out)
}

int oracle_seq_posterior(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                         const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h, int64_t sh,
                         const double *R, int64_t sR, const double *y, const double *x0m, const double *x0P,
                         double *G, double *g, double *L, double *xfm, double *xfP) {
    DISPATCH(seq_posterior, T, A, sA, a, sa, Q, sQ, H, sH, h, sh, R, sR, y, x0m, x0P, G, g, L, xfm, xfP)
}

int oracle_seq_posterior_marginals(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                                   const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h,
                                   int64_t sh, const double *R, int64_t sR, const double *y,
                                   const double *x0m, const double *x0P, const double *Rnew, int64_t sRn,
                                   double *G, double *g, double *L, double *mean_out, double *var_out) {
    DISPATCH(seq_posterior_marginals, T, A, sA, a, sa, Q, sQ, H, sH, h, sh, R, sR, y, x0m, x0P, Rnew, sRn,
             G, g, L, mean_out, var_out)
}

int oracle_seq_prior_marginals(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                               const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h,
                               int64_t sh, const double *R, int64_t sR, const double *x0m, const double *x0P,
                               double *mean_out, double *var_out) {
    DISPATCH(seq_prior_marginals, T, A, sA, a, sa, Q, sQ, H, sH, h, sh, R, sR, x0m, x0P, mean_out, var_out)
}

int oracle_seq_rand(int d, int64_t T, const double *A, int64_t sA, const double *a, int64_t sa,
                    const double *Q, int64_t sQ, const double *H, int64_t sH, const double *h, int64_t sh,
                    const double *R, int64_t sR, const double *x0m, const double *x0P,
                    const double *eps_t, const double *eps_e, const double *eps_0, double *y_out) {
    DISPATCH(seq_rand, T, A, sA, a, sa, Q, sQ, H, sH, h, sh, R, sR, x0m, x0P, eps_t, eps_e, eps_0, y_out)
}
