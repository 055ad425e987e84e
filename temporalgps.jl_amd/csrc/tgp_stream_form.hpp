// The input-normalised modal form the two streaming kernels run on (tgp_lml.hip, tgp_post.hip).  Plain C++: used by the kernels' host
// code and by a host-only test (tests/test_stream_form_host.py).
//
// The plan (tgp_steady_plan.hpp Modal) leaves the basis inside every block of the modal form free.  Here it is fixed by where the input enters:
//   forward   z = B (x + s):  B scales every block by its own input coefficient -- a conjugate pair, read as one complex state, by the complex number
//             its (fb_0, fb_1) stand for, a real mode by its fb -- and s is the fixed point of what is left of the affine part.  The recursion becomes
//                 x' = M x + e u~,   r = u~ - w~ . x,   u~ = y - h~,     e = (1, 0) on a pair, 1 on a real mode,
//             with w~ = fw B (a row times the blocks), (I - M - e w~') s = B^-1 fa and h~ = hh + w~ . s: no coefficient on the input, no constant.
//   backward  zeta = C xi:  the same scaling by the blocks' gc.  xi' = Mg xi + e r,  mean = y - rS r + (gw C) . xi.  (No shift: no constant.)
// B and C are block scalars: they commute with M and Mg, so the rotation-scaling blocks, every power table and the runs' exchange records stay what they
// were, and the conditioning of the modal form is the plan's.  The result is again a Modal -- fb, gc in {0, 1}, fa = 0, hh = h~ -- so everything on the
// host that works from a Modal (the kernels' tables, quad_table, finish) works on it as it is; only what crosses the kernels' boundary is mapped:
// state_in (the head's end state), zeta_out (the backward state handed to the head).
// A block the observation barely excites cannot be normalised by its input: |coefficient| below kRelMin of the largest, or anything not finite, and
// the form declines (the caller stays on k_steady_one, in the plan's coordinates).
#pragma once
#include "tgp_steady_plan.hpp"

#include <cmath>

namespace tgp_stream_form {

constexpr int kMaxD = tgp_plan::kMaxD;
constexpr double kRelMin = 1e-8;
// The streaming logpdf kernel closes its first tile on the host as a quadratic form in the head's end state: sum (r0_t - w_t . x)^2 expanded into
// sum r0_t^2 - 2 x . sum r0_t w_t + x' W x.  Its rounding is eps times the size of the terms, not of the result.  With the input entering every block
// with coefficient 1 a block settles at u / (1 - lambda_i), so the terms are (amp u)^2 with amp = sum_i |w~_i| / |1 - lambda_i|, while the innovations
// are of the size of u or below: the closure loses amp^2.  Ordinary models have amp = 1 .. 6; a closed loop whose real modes nearly coincide has w~ in
// the thousands with alternating signs (a Matern-5/2 model 1e-6 in the spacing from the point where its pair splits: amp = 1.9e3, logpdf off by 1.5e-9
// absolute).  64^2 eps = 4.5e-13 leaves a factor 200 for u^2 / S and a small |logpdf| under the 1e-10 bar; beyond it k_steady_one serves logpdf.
constexpr double kClosureAmpMax = 64.0;

struct Form {
    bool ok = false;
    tgp_plan::Modal md{};               // the normal form (d, n0, nhs, n1, halo, npair, rS, iS, logS, LS, vb, fd, fo, gd, go: the plan's)
    double bp[kMaxD], bq[kMaxD];        // B: the block [[p, q], [-q, p]] of a pair (both members carry it), p alone (q = 0) on a real mode
    double cp[kMaxD], cq[kMaxD];        // C likewise
    double s[kMaxD];                    // the forward shift, in the kernels' coordinates
    double amp = 0.0;                   // sum_i |w~_i| / |1 - lambda_i|: what the logpdf kernel's quadratic closure amplifies rounding by (kClosureAmpMax)
};

namespace detail {
inline int partner(int i, int np) { return i < 2 * np ? (i ^ 1) : i; }
// out = P x, P the block scalar (p, q): a pair's members (x_0, x_1) -> (p x_0 + q x_1, -q x_0 + p x_1)
inline void apply(int d, int np, const double* p, const double* q, const double* x, double* out) {
    for (int i = 0; i < d; ++i) {
        const int k = partner(i, np);
        out[i] = k == i ? p[i] * x[i] : ((i & 1) ? p[i] * x[i] - q[i] * x[k] : p[i] * x[i] + q[i] * x[k]);
    }
}
// out = P^-1 x
inline void apply_inv(int d, int np, const double* p, const double* q, const double* x, double* out) {
    for (int i = 0; i < d; ++i) {
        const int k = partner(i, np);
        if (k == i) out[i] = x[i] / p[i];
        else {
            const double n2 = p[i] * p[i] + q[i] * q[i];
            out[i] = ((i & 1) ? p[i] * x[i] + q[i] * x[k] : p[i] * x[i] - q[i] * x[k]) / n2;
        }
    }
}
// out = w P (a row vector times the blocks)
inline void row_apply(int d, int np, const double* p, const double* q, const double* w, double* out) {
    for (int i = 0; i < d; ++i) {
        const int k = partner(i, np);
        out[i] = k == i ? w[i] * p[i] : ((i & 1) ? w[i] * p[i] + w[k] * q[i] : w[i] * p[i] - w[k] * q[i]);
    }
}
// the block scalar that carries (1, 0) to a pair's coefficients (c_0, c_1): p = c_0, q = -c_1; a real mode: p = c.  false: the guard
inline bool scaling(int d, int np, const double* c, double* p, double* q) {
    double mag[kMaxD], top = 0.0;
    for (int i = 0; i < d; ++i) {
        const int k = partner(i, np);
        if (k == i) {
            p[i] = c[i];
            q[i] = 0.0;
            mag[i] = std::fabs(c[i]);
        } else {
            const int e = i & ~1;
            p[i] = c[e];
            q[i] = -c[e + 1];
            mag[i] = std::sqrt(c[e] * c[e] + c[e + 1] * c[e + 1]);
        }
        if (!std::isfinite(mag[i])) return false;
        top = mag[i] > top ? mag[i] : top;
    }
    for (int i = 0; i < d; ++i)
        if (!(mag[i] >= kRelMin * top) || !(mag[i] > 0.0)) return false;
    return true;
}
// A s = b by elimination with partial pivoting (n <= kMaxD, row-major; A and b are used up).  false: singular to working precision
inline bool solve(int n, double* A, double* b, double* s) {
    double top = 0.0;
    for (int i = 0; i < n * n; ++i) top = std::fabs(A[i]) > top ? std::fabs(A[i]) : top;
    for (int c = 0; c < n; ++c) {
        int piv = c;
        for (int r = c + 1; r < n; ++r)
            if (std::fabs(A[r * n + c]) > std::fabs(A[piv * n + c])) piv = r;
        if (!(std::fabs(A[piv * n + c]) > 1e-12 * top)) return false;
        if (piv != c) {
            for (int k = 0; k < n; ++k) std::swap(A[c * n + k], A[piv * n + k]);
            std::swap(b[c], b[piv]);
        }
        for (int r = c + 1; r < n; ++r) {
            const double f = A[r * n + c] / A[c * n + c];
            for (int k = c; k < n; ++k) A[r * n + k] -= f * A[c * n + k];
            b[r] -= f * b[c];
        }
    }
    for (int r = n - 1; r >= 0; --r) {
        double v = b[r];
        for (int k = r + 1; k < n; ++k) v -= A[r * n + k] * s[k];
        s[r] = v / A[r * n + r];
    }
    return true;
}
}  // namespace detail

// The plan's modal form -> the normal form.  false (and f.ok = false): the streaming kernels decline this model.
inline bool build(const tgp_plan::Modal& in, Form& f) {
    using namespace detail;
    f.ok = false;
    f.md = in;
    const int d = in.d, np = in.npair;
    if (d < 1 || d > kMaxD) return false;
    // (a pair is a rotation-scaling block: what makes a block scalar commute with it)
    for (int i = 0; i + 1 < 2 * np; i += 2)
        if (in.fd[i] != in.fd[i + 1] || in.fo[i] != -in.fo[i + 1] || in.gd[i] != in.gd[i + 1] || in.go[i] != -in.go[i + 1]) return false;
    if (!scaling(d, np, in.fb, f.bp, f.bq) || !scaling(d, np, in.gc, f.cp, f.cq)) return false;
    tgp_plan::Modal& md = f.md;
    row_apply(d, np, f.bp, f.bq, in.fw, md.fw);
    row_apply(d, np, f.cp, f.cq, in.gw, md.gw);
    for (int i = 0; i < d; ++i) {
        const bool second = partner(i, np) != i && (i & 1);      // the second member of a conjugate pair: the input enters through the first
        md.fb[i] = md.gc[i] = second ? 0.0 : 1.0;
        md.fa[i] = 0.0;
        f.s[i] = 0.0;
    }
    bool affine = false;
    for (int i = 0; i < d; ++i) affine = affine || in.fa[i] != 0.0;
    if (affine) {
        // (I - M - e w~') s = B^-1 fa
        double A[kMaxD * kMaxD], b[kMaxD];
        apply_inv(d, np, f.bp, f.bq, in.fa, b);
        for (int i = 0; i < d; ++i)
            for (int k = 0; k < d; ++k) {
                double m = i == k ? in.fd[i] : (k == partner(i, np) ? in.fo[i] : 0.0);
                A[i * d + k] = (i == k ? 1.0 : 0.0) - m - md.fb[i] * md.fw[k];
            }
        if (!solve(d, A, b, f.s)) return false;
    }
    f.amp = 0.0;
    for (int i = 0; i < d; ++i) f.amp += std::fabs(md.fw[i]) / std::sqrt((1.0 - in.fd[i]) * (1.0 - in.fd[i]) + in.fo[i] * in.fo[i]);
    double hs = in.hh;
    for (int i = 0; i < d; ++i) hs += md.fw[i] * f.s[i];
    md.hh = hs;
    for (int i = 0; i < d; ++i)
        if (!std::isfinite(md.fw[i]) || !std::isfinite(md.gw[i]) || !std::isfinite(f.s[i])) return false;
    if (!std::isfinite(md.hh)) return false;
    // the power tables the plan carries for k_steady_one (fp8, WJ, ...) belong to its coordinates: the streaming kernels build their own from fd, fo, fw, gw
    f.ok = true;
    return true;
}

// a forward state of the plan (the head's end state) in the kernels' coordinates: x = B^-1 z - s
inline void state_in(const Form& f, const double* z, double* x) {
    detail::apply_inv(f.md.d, f.md.npair, f.bp, f.bq, z, x);
    for (int i = 0; i < f.md.d; ++i) x[i] -= f.s[i];
}
// ... and back: z = B (x + s)
inline void state_out(const Form& f, const double* x, double* z) {
    double t[kMaxD];
    for (int i = 0; i < f.md.d; ++i) t[i] = x[i] + f.s[i];
    detail::apply(f.md.d, f.md.npair, f.bp, f.bq, t, z);
}
// a backward state of the kernels in the plan's coordinates (what the head's backward recursion starts from): zeta = C xi
inline void zeta_out(const Form& f, const double* xi, double* zeta) { detail::apply(f.md.d, f.md.npair, f.cp, f.cq, xi, zeta); }

}  // namespace tgp_stream_form
