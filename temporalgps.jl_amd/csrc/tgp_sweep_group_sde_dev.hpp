// Device half shared by the group sweep's two units for SDE-described models (tgp_sweep_group_sde.hip: logpdf and posterior marginals, DESIGN 4.13;
// tgp_sweep_group_adjoint_sde.hip: the adjoint gradient): the kernels' argument block, the rows with the gaps, the transition of a step
// as a lane applies it, the lane (LaneS) and the forward run.  Private to those two units.
#pragma once
#include "tgp_sweep_group_dev.hpp"

namespace tgp_sweep_group {

struct GSArgs {
    GArgs ka;      // (ka.mc: gP = Pinf, (x0m, x0P) = the state in front of update 0; ka.st.tau: the gaps)
    tgp_sweep::GroupSdeC sc;
};
static_assert(sizeof(GSArgs) <= 4096, "the kernel's argument segment");

constexpr int kBand = tgp_sweep::kGroupSdeBand;

// Row with the gaps beside y: tau[t] = the gap in FRONT of step t (entry 0 unused: the first transition is the host's)
template <int XS> struct RowS : Row<XS> {
    double tau;
};
template <int XS> __device__ __forceinline__ void load_row_s(const GArgs& ka, long long tb, int j, RowS<XS>& r) {
    load_row<XS>(ka, tb, j, r);
    r.tau = ka.st.tau[tgp_sweep::clamp_t(tb + j, ka.T)];
}

// The transition of one step as a lane applies it: the gap and one exponential per distinct lam (wave-uniform comparisons, as step_A)
template <int D> struct StepA {
    double tau, e[D];
};

template <int D, int XS> struct LaneS : Lane<D, XS, false> {
    using Lane<D, XS, false>::j;
    using Lane<D, XS, false>::act;
    using Lane<D, XS, false>::tile;
    using Lane<D, XS, false>::H;
    using Lane<D, XS, false>::aj;
    const double* sN1;      // N1, N2 in LDS, row-major [8 i + k], zero outside d x d   (the base's sA and Qc are not used)
    const double* sN2;
    double lam[D];          // wave-uniform
    double Gc[D];           // column j of Pinf

    __device__ __forceinline__ void step_A(double tau, StepA<D>& s) const {
        s.tau = tau;
        s.e[0] = ::exp(-lam[0] * tau);
        TGP_GU for (int i = 1; i < D; ++i) s.e[i] = (lam[i] == lam[i - 1]) ? s.e[i - 1] : ::exp(-lam[i] * tau);
    }
    // y[:, j] = A_t x[:, j]
    __device__ __forceinline__ void mul_A(const StepA<D>& s, const double* x, double* y) const {
        TGP_GU for (int i = 0; i < D; ++i) {
            double u = 0.0, w = 0.0;
            TGP_GU for (int k = (i > kBand ? i - kBand : 0); k <= (i + kBand < D - 1 ? i + kBand : D - 1); ++k) {
                u = fma(sN1[G * i + k], x[k], u);
                w = fma(sN2[G * i + k], x[k], w);
            }
            y[i] = s.e[i] * fma(s.tau, fma(s.tau, w, u), x[i]);
        }
    }
    // predict:  m <- A m + a,  P <- Pinf + A (P - Pinf) A'.  Lane::predict's one trip through the tile.  AP (optional): column j of A P of the INCOMING
    // covariance; then W = A P - A Pinf, the two products formed separately.
    __device__ __forceinline__ void predict(const StepA<D>& s, GState<D>& x, double* AP = nullptr) const {
        double W[D], row[D], v[D];
        if (AP) {
            double AG[D];
            mul_A(s, x.P, AP);
            mul_A(s, Gc, AG);
            TGP_GU for (int i = 0; i < D; ++i) W[i] = AP[i] - AG[i];
        } else {
            double Dc[D];
            TGP_GU for (int i = 0; i < D; ++i) Dc[i] = x.P[i] - Gc[i];
            mul_A(s, Dc, W);
        }
        wave_sync();
        TGP_GU for (int i = 0; i < D; ++i) tile[i + G * j] = W[i];
        tile[V0 + j] = x.m;
        wave_sync();
        TGP_GU for (int k = 0; k < D; ++k) {
            row[k] = act ? tile[j + G * k] : 0.0;      // rows >= D of the tile are never written
            v[k] = tile[V0 + k];
        }
        mul_A(s, row, x.P);
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] += Gc[i];
        // the mean's row j: this lane's own row of N1 / N2 (zero in a padding lane) and e_j by selects (no indexing of registers by the lane).  All d
        // columns, not the band of mul_A: there the row i is a compile-time index and so is its band, here the row is the lane's j, known only at run
        // time -- the entries outside the band are the zeros the plan has checked
        double u = 0.0, w = 0.0, ej = s.e[0];
        TGP_GU for (int k = 0; k < D; ++k) {
            u = fma(sN1[G * j + k], v[k], u);
            w = fma(sN2[G * j + k], v[k], w);
            ej = (j == k) ? s.e[k] : ej;
        }
        x.m = fma(ej, fma(s.tau, fma(s.tau, w, u), x.m), aj);
    }
    // one step of the filter with step k of a row's inputs; at t == 0 the state is the host's (the prior through the first transition): kept
    __device__ __forceinline__ void fstep(GState<D>& x, const RowS<XS>& r, int k, long long t, long long T, LmlAcc* acc, bool& ok) const {
        const double y = __shfl(r.y, k, G);
        const double Rt = (XS & 1) ? __shfl(r.R, k, G) : this->R;
        const double ht = (XS & 2) ? __shfl(r.hh, k, G) : this->hh;
        const bool obs = t < T && __shfl((int)r.mk, k, G) == 0;
        const double tau = __shfl(r.tau, k, G);
        StepA<D> s;
        step_A(t <= 0 ? 0.0 : tau, s);
        const GState<D> keep = x;
        predict(s, x);
        if (t == 0) x = keep;
        this->update(x, y, Rt, ht, obs, acc, ok);
    }
    // Lane::smooth_step with the transition of step t + 1 (s).  Behind the predict this is that function's body, line for line, and the two must stay in
    // step: it is repeated here, not shared, because a helper cut out of Lane::smooth_step would have to leave the 64 recorded resource lines of
    // tgp_sweep_group.hip's kernels where they are (profiles/sweep_group*_resources.txt).
    __device__ __forceinline__ void smooth_step(const StepA<D>& s, const GState<D>& xf, GState<D>& xs, bool& ok) const {
        GState<D> xp = xf;
        double AP[D];
        predict(s, xp, AP);
        double Xc[D];
        this->gain_cols(xp.P, AP, Xc, ok);
        double dm[D];
        this->gather(xs.m - xp.m, dm, V0);
        double accm = xf.m;
        TGP_GU for (int k = 0; k < D; ++k) accm = fma(Xc[k], dm[k], accm);
        xs.m = accm;
        double Dm[D], N[D];
        TGP_GU for (int i = 0; i < D; ++i) Dm[i] = act ? xs.P[i] - xp.P[i] - ((i == j) ? kJitter : 0.0) : 0.0;
        this->publish(Xc);
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_GU for (int k = 0; k < D; ++k) acc = fma(tile[k + G * i], Dm[k], acc);
            N[i] = acc;
        }
        this->publish(N);
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = xf.P[i];
            TGP_GU for (int k = 0; k < D; ++k) acc = fma(tile[i + G * k], Xc[k], acc);
            xs.P[i] = act ? acc : 0.0;
        }
    }
};

// tgp_sweep_group.hip forward_run with the gaps in the rows (step loops rolled in both calls: nothing of A_t could stay in registers across steps)
template <int D, int XS, int B>
__device__ __forceinline__ void forward_run_s(const GArgs& ka, const LaneS<D, XS>& ln, long long ts, int nrows, long long lo, long long hi, GState<D>& x, LmlAcc& acc,
                                              bool want_lml, double* ck, long long ck_t0, size_t ck_ld, bool& ok) {
    RowS<XS> in, nx;
    load_row_s<XS>(ka, ts, ln.j, in);
    for (int r = 0; r < nrows; ++r) {
        const long long tb = ts + 8ll * r;
        load_row_s<XS>(ka, tb + 8, ln.j, nx);      // in flight while this row computes (behind the last row: clamped, unused)
        if (tb >= lo && tb < hi) {
#pragma nounroll
            for (int k = 0; k < 8; ++k) {
                if (ck != nullptr && k % B == 0) ln.store_packed(ck + (size_t)((tb + k - ck_t0) / B) * ck_ld, x);
                ln.fstep(x, in, k, tb + k, ka.T, &acc, ok);
            }
        }
        if (want_lml) acc.flush();
        else acc.prod = 1.0;
        in = nx;
    }
}
}  // namespace tgp_sweep_group
