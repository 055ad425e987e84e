// Host half of the adjoint gradient of logpdf for WIDE models (8 < d <= 63, the wide-state engine's class: tgp_wide.hip) -- the algorithm and the
// record layout of tgp_adjoint::finish (tgp_adjoint_host.hpp), arranged for d up to 63:
//   * the covariance recursion is not re-iterated when the caller hands the plan's kept head over (gains K_t, innovation variances S_t, filtered
//     covariances Pf_t for t = 0 .. n0): the predicted covariance is Pp_t = Pf_t + v_t v_t' / S_t with v_t = K_t S_t, the previous one Pf_(t-1)
//     (x0P at t = 0) -- O(d^2) per step instead of O(d^3);
//   * the reverse sweep's four d x d products per step run as row-major i-k-j loops (vectorised: the including object is built with AVX2 + FMA, and
//     checks the CPU for them at run time);
//   * the head is `head_steps` long (the wide engine's n0 + 1 steps, not 512-step tiles).
// Cost: O(head_steps d^2) for the head's means, 4 d^3 multiply-adds per covariance step for the reverse sweep (d = 42, 300 steps: ~9e7).
#pragma once
#include <cstdint>
#include <vector>

#include "tgp_adjoint_host.hpp"

namespace tgp_wide_adjoint {

struct Head {      // the plan's kept head, row-major: K [n][d], S [n], Pf [n][d d] with n >= record n0 + 1 (Pf == nullptr: re-iterate the covariances)
    const double *K = nullptr, *S = nullptr, *Pf = nullptr;
    int64_t n = 0;
};

namespace detail {
inline void mm(int d, const double* X, const double* Y, double* Z) {      // Z = X Y
    for (int i = 0; i < d; ++i) {
        double* zi = Z + (size_t)i * d;
        for (int j = 0; j < d; ++j) zi[j] = 0.0;
        for (int k = 0; k < d; ++k) {
            const double x = X[(size_t)i * d + k];
            const double* yk = Y + (size_t)k * d;
            for (int j = 0; j < d; ++j) zi[j] += x * yk[j];
        }
    }
}
inline void mm_tn(int d, const double* X, const double* Y, double* Z) {      // Z = X' Y
    for (size_t e = 0; e < (size_t)d * d; ++e) Z[e] = 0.0;
    for (int k = 0; k < d; ++k) {
        const double* xk = X + (size_t)k * d;
        const double* yk = Y + (size_t)k * d;
        for (int i = 0; i < d; ++i) {
            const double x = xk[i];
            double* zi = Z + (size_t)i * d;
            for (int j = 0; j < d; ++j) zi[j] += x * yk[j];
        }
    }
}
inline void mm_acc(int d, const double* X, const double* Y, double* Z) {      // Z += X Y
    for (int i = 0; i < d; ++i) {
        double* zi = Z + (size_t)i * d;
        for (int k = 0; k < d; ++k) {
            const double x = X[(size_t)i * d + k];
            const double* yk = Y + (size_t)k * d;
            for (int j = 0; j < d; ++j) zi[j] += x * yk[j];
        }
    }
}
}  // namespace detail

// rec: tgp_adjoint::record_size(d) doubles (meta: n0 = the index of the settled gain, head tiles ignored, T, applies); yh: the first nyh >= head_steps
// observations.  Returns 0, or 1 when the record says the engine did not apply / the arguments do not fit it.
inline int finish(int d, const double* rec, const double* yh, int64_t nyh, int64_t head_steps, const tgp_adjoint::Out& out, const Head* head = nullptr) {
    using namespace detail;
    const int DD = d * d, NS = DD + 3 * d + 2;
    const double *SA = rec, *Sa = rec + DD, *Sk = rec + DD + d, *Srm = rec + DD + 2 * d;
    const double Sr = rec[DD + 3 * d], SSQ = rec[DD + 3 * d + 1];
    const double *psi_nh = rec + NS, *meta = rec + NS + 2 * d, *md = meta + 4;
    const int64_t n0 = (int64_t)meta[0], T = (int64_t)meta[2];
    if (meta[3] != 1.0 || n0 < 0 || head_steps < 0) return 1;
    const int64_t nh = head_steps;
    if (nyh < nh || nh > T) return 1;
    const int64_t ns = n0 + 1;
    if (head && head->n < ns) head = nullptr;
    std::vector<double> A(DD), Q(DD), a(d), h(d), x0m(d), P0(DD);
    for (int i = 0; i < d; ++i) {
        for (int k = 0; k < d; ++k) {
            A[i * d + k] = md[i + k * d];
            Q[i * d + k] = md[DD + d + i + k * d];
        }
        a[i] = md[DD + i];
        h[i] = md[2 * DD + d + i];
    }
    const double hh = md[2 * DD + 2 * d], R = md[2 * DD + 2 * d + 1];
    const double* x0 = md + 2 * DD + 2 * d + 2;
    for (int i = 0; i < d; ++i) x0m[i] = x0[i];
    for (int c = 0; c < d; ++c)
        for (int r = 0; r <= c; ++r) P0[r * d + c] = P0[c * d + r] = x0[d + c * (c + 1) / 2 + r];
    // ---- the covariance recursion's steps 0 .. n0: K_t, S_t, Pf_t (handed over, or iterated here)
    std::vector<double> Kown, Sown, Pown;
    const double *Kt = nullptr, *St = nullptr, *Pft = nullptr;
    if (head && head->Pf) {
        Kt = head->K;
        St = head->S;
        Pft = head->Pf;
    } else {
        Kown.resize(ns * d);
        Sown.resize(ns);
        Pown.resize(ns * DD);
        std::vector<double> P(P0), AP(DD), Pp(DD), v(d);
        for (int64_t t = 0; t < ns; ++t) {
            mm(d, A.data(), P.data(), AP.data());
            for (int i = 0; i < d; ++i)
                for (int j = 0; j <= i; ++j) {
                    const double *x = &AP[i * d], *y = &A[j * d];
                    double s = Q[i * d + j];
                    for (int k = 0; k < d; ++k) s += x[k] * y[k];
                    Pp[i * d + j] = Pp[j * d + i] = s;
                }
            double s = R;
            for (int i = 0; i < d; ++i) {
                double x = 0.0;
                for (int k = 0; k < d; ++k) x += Pp[i * d + k] * h[k];
                v[i] = x;
                s += h[i] * x;
            }
            Sown[t] = s;
            for (int i = 0; i < d; ++i) Kown[t * d + i] = v[i] / s;
            for (int i = 0; i < d; ++i)
                for (int j = 0; j < d; ++j) P[i * d + j] = Pp[i * d + j] - v[i] * v[j] / s;
            for (int e = 0; e < DD; ++e) Pown[t * DD + e] = P[e];
        }
        Kt = Kown.data();
        St = Sown.data();
        Pft = Pown.data();
        if (head) {      // (the gains the engine ran with: its own, where it kept them)
            Kt = head->K;
            St = head->S;
        }
    }
    std::vector<double> kA(ns * d);
    for (int64_t t = 0; t < ns; ++t)
        for (int i = 0; i < d; ++i) {
            double x = 0.0;
            for (int k = 0; k < d; ++k) x += A[i * d + k] * Kt[t * d + k];
            kA[t * d + i] = x;
        }
    // ---- head: forward means and innovations
    std::vector<double> mus(nh * d), r(nh), mu(d), nm(d);
    for (int i = 0; i < d; ++i) {
        double x = a[i];
        for (int k = 0; k < d; ++k) x += A[i * d + k] * x0m[k];
        mu[i] = x;
    }
    for (int64_t t = 0; t < nh; ++t) {
        const int64_t ix = t < n0 ? t : n0;
        double rr = yh[t] - hh;
        for (int k = 0; k < d; ++k) {
            mus[t * d + k] = mu[k];
            rr -= h[k] * mu[k];
        }
        r[t] = rr;
        for (int i = 0; i < d; ++i) {
            double x = a[i] + kA[ix * d + i] * rr;
            for (int k = 0; k < d; ++k) x += A[i * d + k] * mu[k];
            nm[i] = x;
        }
        mu.swap(nm);
    }
    // ---- accumulators, seeded with the device's sums over the steps behind the head (all of them at index n0)
    std::vector<double> bA(DD), ba(d), bQ(DD, 0.0), bh(d), bkA(ns * d, 0.0), bS(ns, 0.0), psi(d), np(d);
    double bhh, bR = 0.0;
    const double Sn = St[n0];
    for (int e = 0; e < DD; ++e) bA[e] = SA[e];
    for (int i = 0; i < d; ++i) {
        ba[i] = Sa[i];
        bkA[n0 * d + i] = Sk[i];
        double x = -Srm[i] / Sn;
        for (int k = 0; k < d; ++k) x += SA[k * d + i] * kA[n0 * d + k];
        bh[i] = -x;
    }
    {
        double x = -Sr / Sn;
        for (int k = 0; k < d; ++k) x += kA[n0 * d + k] * Sa[k];
        bhh = -x;
    }
    bS[n0] = -0.5 * ((double)(T - nh) / Sn - SSQ / (Sn * Sn));
    // ---- head, backwards (the rank-one terms psi mu_t' summed as one product at the end)
    std::vector<double> psis(nh * d);
    for (int i = 0; i < d; ++i) psi[i] = psi_nh[i];
    for (int64_t t = nh - 1; t >= 0; --t) {
        const int64_t ix = t < n0 ? t : n0;
        const double rr = r[t], s = St[ix];
        double rho = -rr / s;
        for (int i = 0; i < d; ++i) {
            psis[t * d + i] = psi[i];
            bkA[ix * d + i] += psi[i] * rr;
            ba[i] += psi[i];
            rho += kA[ix * d + i] * psi[i];
        }
        for (int k = 0; k < d; ++k) bh[k] -= rho * mus[t * d + k];
        bhh -= rho;
        bS[ix] += -0.5 * (1.0 / s - rr * rr / (s * s));
        for (int i = 0; i < d; ++i) np[i] = -h[i] * rho;
        for (int k = 0; k < d; ++k) {
            const double pk = psi[k];
            const double* ak = &A[k * d];
            for (int i = 0; i < d; ++i) np[i] += ak[i] * pk;
        }
        psi.swap(np);
    }
    for (int64_t t = 0; t < nh; ++t)      // bA += sum_t psi_(t+1) mu_t'
        for (int i = 0; i < d; ++i) {
            const double p = psis[t * d + i];
            const double* m = &mus[t * d];
            double* row = &bA[i * d];
            for (int k = 0; k < d; ++k) row[k] += p * m[k];
        }
    for (int i = 0; i < d; ++i) {
        ba[i] += psi[i];
        for (int k = 0; k < d; ++k) bA[i * d + k] += psi[i] * x0m[k];
    }
    if (out.gx0m)
        for (int i = 0; i < d; ++i) {
            double x = 0.0;
            for (int k = 0; k < d; ++k) x += A[k * d + i] * psi[k];
            out.gx0m[i] = x;
        }
    // ---- reverse sweep through the covariance recursion
    std::vector<double> bPf(DD, 0.0), bPp(DD), bv(d), bK(d), vt(d), pp(DD), t1(DD), t3(DD);
    for (int64_t t = ns - 1; t >= 0; --t) {
        const double *Kv = &Kt[t * d], *Pf = &Pft[t * DD], *Pq = t > 0 ? &Pft[(t - 1) * DD] : P0.data();
        const double s = St[t];
        double bSt = bS[t];
        for (int i = 0; i < d; ++i) vt[i] = Kv[i] * s;
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < d; ++k) pp[i * d + k] = Pf[i * d + k] + vt[i] * vt[k] / s;
        // Pf = Pp - v v' / S
        for (int e = 0; e < DD; ++e) bPp[e] = bPf[e];
        double q = 0.0;
        for (int i = 0; i < d; ++i) {
            double x = 0.0;
            for (int k = 0; k < d; ++k) {
                x += (bPf[i * d + k] + bPf[k * d + i]) * vt[k];
                q += vt[i] * bPf[i * d + k] * vt[k];
            }
            bv[i] = -x / s;
        }
        bSt += q / (s * s);
        // kA = A K, K = v / S
        double kv = 0.0;
        for (int i = 0; i < d; ++i) bK[i] = 0.0;
        for (int k = 0; k < d; ++k) {
            const double bk = bkA[t * d + k];
            const double* ak = &A[k * d];
            double* brow = &bA[k * d];
            for (int i = 0; i < d; ++i) {
                bK[i] += ak[i] * bk;
                brow[i] += bk * Kv[i];
            }
        }
        for (int i = 0; i < d; ++i) {
            bv[i] += bK[i] / s;
            kv += bK[i] * vt[i];
        }
        bSt -= kv / (s * s);
        // S = h' v + R
        for (int i = 0; i < d; ++i) {
            bh[i] += bSt * vt[i];
            bv[i] += bSt * h[i];
        }
        bR += bSt;
        // v = Pp h
        for (int i = 0; i < d; ++i) {
            const double b = bv[i];
            const double* pr = &pp[i * d];
            double* row = &bPp[i * d];
            for (int k = 0; k < d; ++k) {
                row[k] += b * h[k];
                bh[k] += pr[k] * b;
            }
        }
        // Pp = A Symmetric(P) A' + Q
        for (int e = 0; e < DD; ++e) bQ[e] += bPp[e];
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < d; ++k) t3[i * d + k] = bPp[i * d + k] + bPp[k * d + i];
        mm(d, t3.data(), A.data(), t1.data());
        mm_acc(d, t1.data(), Pq, bA.data());
        mm_tn(d, A.data(), bPp.data(), t1.data());
        mm(d, t1.data(), A.data(), bPf.data());
    }
    // ---- outputs (column-major; symmetric blocks symmetrised)
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < d; ++k) {
            if (out.gA) out.gA[i + k * d] = bA[i * d + k];
            if (out.gQ) out.gQ[i + k * d] = 0.5 * (bQ[i * d + k] + bQ[k * d + i]);
            if (out.gx0P) out.gx0P[i + k * d] = 0.5 * (bPf[i * d + k] + bPf[k * d + i]);
        }
    for (int i = 0; i < d; ++i) {
        if (out.ga) out.ga[i] = ba[i];
        if (out.gH) out.gH[i] = bh[i];
    }
    if (out.ghh) *out.ghh = bhh;
    if (out.gR) *out.gR = bR;
    return 0;
}

}  // namespace tgp_wide_adjoint
