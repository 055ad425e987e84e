// Device half shared by the group sweep's translation units (tgp_sweep_group.hip: the LTI kernels; tgp_sweep_group_sde.hip: the SDE-described models,
// DESIGN 4.13): the kernels' argument block, the 8-lane building blocks and a lane's view of its group (Lane).  Private to those two units.
#pragma once
#include "tgp_sweep_group.hpp"

namespace tgp_sweep_group {

using tgp_sweep::fast_rcp;
using tgp_sweep::fast_sqrt_rsqrt;
using tgp_sweep::GroupModelC;
using tgp_sweep::kJitter;
using tgp_sweep::LmlAcc;

struct GArgs {
    GroupModelC mc;
    tgp_sweep::Streams st;
    long long T;
    int C, W, Wb, owned;
    long long nchunks;
    double* mean;
    double* var;
    double* ckpt;      // [wave][block][group][NS]: the state in front of every block of B steps (posterior calls)
    double* part;      // [wave][4]: share of the log marginal likelihood, status bits, forward / backward distance (pinned host memory)
};
static_assert(sizeof(GArgs) <= 4096, "the kernel's argument segment");

constexpr int G = tgp_sweep::kGroupLanes;
constexpr int kTileLD = G * G + 2 * G + 2;      // tgp_group.hpp GroupGeom::LD: an 8 x 8 matrix (i + 8 col), two 8-vectors, 2 doubles of padding
constexpr int V0 = G * G, V1 = G * G + G;

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
template <int CTRL> __device__ __forceinline__ double dpp_move(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// sum over the 8 lanes of a group, every lane ending with the same bits (tgp_group.hpp group_sum)
__device__ __forceinline__ double group_sum(double x) {
    x += dpp_move<0xB1>(x);       // quad_perm:[1,0,3,2]
    x += dpp_move<0x4E>(x);       // quad_perm:[2,3,0,1]
    x += dpp_move<0x141>(x);      // row_half_mirror
    return x;
}
__device__ __forceinline__ double group_max(double x) {
    double o = dpp_move<0xB1>(x);
    x = o > x ? o : x;
    o = dpp_move<0x4E>(x);
    x = o > x ? o : x;
    o = dpp_move<0x141>(x);
    return o > x ? o : x;
}

#define TGP_GU _Pragma("unroll")

// a state by columns: lane j holds element j of the mean and column j of the covariance
template <int D> struct GState {
    double m;
    double P[D];
};

// a lane's sums of the block gradients over the steps of its group's chunk (k_sweep_group_adjoint): column j of gA and of gQ (full, not packed),
// element j of ga and gH, the sums of the per-step gh_t and gR_t (the same in every lane of the group)
template <int D> struct GAcc {
    double gA[D], gQ[D], ga, gH, gh, gR;
    __device__ __forceinline__ void zero() {
        TGP_GU for (int i = 0; i < D; ++i) gA[i] = gQ[i] = 0.0;
        ga = gH = gh = gR = 0.0;
    }
};

// The 8 steps of a row of the observation stream, one per lane of the group (a 64-byte row per stream and group); handed out step by step with a
// shuffle inside the group.  XS bit 0: the noise variance is per step, bit 1: the emission offset is.
template <int XS> struct Row {
    double y, R, hh;
    unsigned mk;
};
template <int XS> __device__ __forceinline__ void load_row(const GArgs& ka, long long tb, int j, Row<XS>& r) {
    const long long t = tgp_sweep::clamp_t(tb + j, ka.T);
    r.y = ka.st.y[t];
    r.R = (XS & 1) ? ka.st.R[t] : 0.0;
    r.hh = (XS & 2) ? ka.st.hh[t] : 0.0;
    r.mk = ka.st.mask != nullptr ? (unsigned)ka.st.mask[t] : 0u;
}

// KEEP_A: the logpdf kernels (<= 202 registers) unroll the eight steps of a row, and the optimiser keeps A (read from LDS as a wave-wide broadcast) in
// registers across them; the posterior kernels keep their step loops rolled (forward_run, backward_run).
template <int D, int XS, bool KEEP_A> struct Lane {
    static constexpr int NS = D + D * (D + 1) / 2;
    int j;                // lane inside the group == the column it owns
    bool act;             // j < D
    double* tile;         // the group's exchange tile
    const double* sA;     // A in LDS, row-major [8 i + k], zero outside d x d
    double Qc[D], H[D], Hj, aj, hh, R;

    // y[:, j] = A x[:, j]
    __device__ __forceinline__ void mul_A(const double* x, double* y) const {
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_GU for (int k = 0; k < D; ++k) acc = fma(sA[G * i + k], x[k], acc);
            y[i] = acc;
        }
    }
    // every lane gets the D elements of a vector held one element per lane
    __device__ __forceinline__ void gather(double vj, double* v, int at) const {
        wave_sync();
        tile[at + j] = vj;
        wave_sync();
        TGP_GU for (int k = 0; k < D; ++k) v[k] = tile[at + k];
    }
    // tile[i + 8 j] = c[i]: lane j writes column j (rows < D only)
    __device__ __forceinline__ void publish(const double* c) const {
        wave_sync();
        TGP_GU for (int i = 0; i < D; ++i) tile[i + G * j] = c[i];
        wave_sync();
    }
    // predict (lgc.jl:46-52):  m <- A m + a,  P <- A P A' + Q.  W = A P is lane-local; its transpose and the gather of m share ONE trip through
    // the tile; column j of A P A' is A (row j of W)'.  AP (optional): column j of A P of the INCOMING covariance (what invert_dynamics multiplies again).
    __device__ __forceinline__ void predict(GState<D>& x, double* AP = nullptr) const {
        double W[D], row[D], v[D];
        mul_A(x.P, W);
        if (AP) { TGP_GU for (int i = 0; i < D; ++i) AP[i] = W[i]; }
        wave_sync();
        TGP_GU for (int i = 0; i < D; ++i) tile[i + G * j] = W[i];
        tile[V0 + j] = x.m;
        wave_sync();
        TGP_GU for (int k = 0; k < D; ++k) {
            row[k] = act ? tile[j + G * k] : 0.0;      // rows >= D of the tile are never written
            v[k] = tile[V0 + k];
        }
        mul_A(row, x.P);
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] += Qc[i];
        double acc = 0.0;
        TGP_GU for (int k = 0; k < D; ++k) acc = fma(sA[G * j + k], v[k], acc);
        x.m = acc + aj;
    }
    // posterior_and_lml of a ScalarOutputLGC (lgc.jl:247-257); obs == false: the step is missing, nothing changes (tgp_sweep_body.hpp update)
    __device__ __forceinline__ void update(GState<D>& x, double y, double Rt, double ht, bool obs, LmlAcc* acc, bool& ok) const {
        double vj = 0.0;      // V = P H, element j (by symmetry lane-local)
        TGP_GU for (int i = 0; i < D; ++i) vj = fma(x.P[i], H[i], vj);
        const double s2 = group_sum(Hj * vj) + Rt;
        const double hm = group_sum(Hj * x.m) + ht;
        const double S = obs ? s2 : 1.0;
        ok = ok && (S > 0.0);
        const double iS = obs ? fast_rcp(S) : 0.0;
        const double v = obs ? (y - hm) : 0.0;
        const double viS = v * iS;
        x.m = fma(vj, viS, x.m);
        double V[D];
        gather(vj, V, V1);
        const double w = vj * iS;
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] = fma(-V[i], w, x.P[i]);
        if (acc) {
            acc->q = fma(v, viS, acc->q);
            acc->prod *= S;
            acc->n += obs ? 1.0 : 0.0;
        }
    }
    // one step of the filter with step k of a row's inputs
    __device__ __forceinline__ void fstep(GState<D>& x, const Row<XS>& r, int k, long long t, long long T, LmlAcc* acc, bool& ok) const {
        const double y = __shfl(r.y, k, G);
        const double Rt = (XS & 1) ? __shfl(r.R, k, G) : R;
        const double ht = (XS & 2) ? __shfl(r.hh, k, G) : hh;
        const bool obs = t < T && __shfl((int)r.mk, k, G) == 0;      // (steps behind the series are missing: the runs pad their last row)
        predict(x);
        update(x, y, Rt, ht, obs, acc, ok);
    }

    // Upper Cholesky factor of M + jit I by the 8-lane scheme of tgp_group_smooth.hpp (Mc: column j of the symmetric M), one row per step: lane i finishes
    // U[i][i] and hands its column above the diagonal to everybody.  Uc: column j of U (zero below the diagonal and in a padding lane), rinv: the
    // reciprocal pivots (the same in every lane).
    __device__ __forceinline__ void chol_cols(const double* Mc, double jit, double* Uc, double* rinv, bool& ok) const {
        TGP_GU for (int i = 0; i < D; ++i) Uc[i] = 0.0;
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = Mc[i] + ((i == j) ? jit : 0.0);
            wave_sync();
            if (j == i) {
                double dg = acc;
                TGP_GU for (int k = 0; k < i; ++k) dg = fma(-Uc[k], Uc[k], dg);
                double s, rs;
                fast_sqrt_rsqrt(dg, s, rs);
                TGP_GU for (int k = 0; k < i; ++k) tile[V0 + k] = Uc[k];
                tile[V1 + 0] = dg;
                tile[V1 + 1] = s;
                tile[V1 + 2] = rs;
            }
            wave_sync();
            const double dg = tile[V1 + 0], di = tile[V1 + 1];
            rinv[i] = tile[V1 + 2];
            ok = ok && (dg > 0.0);
            TGP_GU for (int k = 0; k < i; ++k) acc = fma(-tile[V0 + k], Uc[k], acc);
            Uc[i] = (j == i) ? di : ((j > i && act) ? acc * rinv[i] : 0.0);
        }
    }
    // The gain of the reverse-time recursion, shared by smooth_step and draw_step: U = the upper factor of Pp + 1e-10 I, left PUBLISHED in the tile
    // (tile[i + 8 k] = U[i][k]), and Xc = column j of G' = (Pp + jitter I)^-1 (A Pf):  U' z = AP[:, j],  U w = z  (zero in a padding lane).
    __device__ __forceinline__ void gain_cols(const double* Ppc, const double* AP, double* Xc, bool& ok) const {
        double Uc[D], rinv[D];
        chol_cols(Ppc, kJitter, Uc, rinv, ok);
        publish(Uc);
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = AP[i];
            TGP_GU for (int k = 0; k < i; ++k) acc = fma(-tile[k + G * i], Xc[k], acc);
            Xc[i] = acc * rinv[i];
        }
        TGP_GU for (int i = D - 1; i >= 0; --i) {
            double acc = Xc[i];
            TGP_GU for (int k = i + 1; k < D; ++k) acc = fma(-tile[i + G * k], Xc[k], acc);
            Xc[i] = acc * rinv[i];
        }
        if (!act) { TGP_GU for (int i = 0; i < D; ++i) Xc[i] = 0.0; }
    }

    // One step of the reverse-time recursion (lgssm.jl:231-238 + :111-115; tgp_sweep_body.hpp smooth_step in the column layout): xf = filtering
    // state of step t, xs = smoothing state of step t + 1 on entry, of step t on return.  G = Pf A' (Pp + 1e-10 I)^-1 by the 8-lane Cholesky of
    // tgp_group_smooth.hpp (gain_cols); gain form  ms = mf + G (ms+ - mp),  Ps = Pf + G (Ps+ - Pp - 1e-10 I) G'.
    __device__ __forceinline__ void smooth_step(const GState<D>& xf, GState<D>& xs, bool& ok) const {
        GState<D> xp = xf;
        double AP[D];
        predict(xp, AP);
        double Xc[D];
        gain_cols(xp.P, AP, Xc, ok);
        // ---- the mean: (G dm)_j = sum_k G'[k][j] dm_k
        double dm[D];
        gather(xs.m - xp.m, dm, V0);
        double accm = xf.m;
        TGP_GU for (int k = 0; k < D; ++k) accm = fma(Xc[k], dm[k], accm);
        xs.m = accm;
        // ---- the covariance: N = G Dm (column j lane-local with G' published: G[i][k] = tile[k + 8 i]), then column j of N G' = N (G')[:, j]
        double Dm[D], N[D];
        TGP_GU for (int i = 0; i < D; ++i) Dm[i] = act ? xs.P[i] - xp.P[i] - ((i == j) ? kJitter : 0.0) : 0.0;
        publish(Xc);
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_GU for (int k = 0; k < D; ++k) acc = fma(tile[k + G * i], Dm[k], acc);
            N[i] = acc;
        }
        publish(N);
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = xf.P[i];
            TGP_GU for (int k = 0; k < D; ++k) acc = fma(tile[i + G * k], Xc[k], acc);
            xs.P[i] = act ? acc : 0.0;
        }
    }
    // emission predict of a smoothing state without the replaced noise (the caller adds it): mean = H' m + h, var = H' P H
    __device__ __forceinline__ void emit(const GState<D>& xs, double ht, double& mean, double& var) const {
        double pj = 0.0;
        TGP_GU for (int i = 0; i < D; ++i) pj = fma(xs.P[i], H[i], pj);
        mean = group_sum(Hj * xs.m) + ht;
        var = group_sum(Hj * pj);
    }

    // ---- a draw from the posterior (k_sweep_group_draw): tgp_sweep_body.hpp draw_start / draw_step_r in the column layout.  The sample
    // state is ONE double per lane: lane j holds x_j (zero in a padding lane).  e[k] = draw k of the step, gathered (the same in every lane).
    // (U' e)_j = sum_(k <= j) U[k][j] e_k: column j of the factor against the gathered draws, lane-local (Uc is zero below the diagonal)
    __device__ __forceinline__ double mul_Ut(const double* Uc, const double* e) const {
        double acc = 0.0;
        TGP_GU for (int k = 0; k < D; ++k) acc = fma(Uc[k], e[k], acc);
        return acc;
    }
    // x_(T-1) = mf + chol(Pf + 1e-12 I).U' eps_0
    __device__ __forceinline__ double draw_start(const GState<D>& xf, const double* e0, bool& ok) const {
        double Uc[D], rinv[D];
        chol_cols(xf.P, tgp_sweep::kJitterStart, Uc, rinv, ok);
        return xf.m + mul_Ut(Uc, e0);
    }
    // One step of the walk: xf = filtering state of step t, e = eps_t[t + 1]; x = x_(t+1) on entry, x_t on return:
    // x_t = mf + G (x_(t+1) - mp) + chol(L + 1e-9 I).U' e,  L = Pf - (U G')'(U G') in the reference's form (lgc.jl:84-87).  The step does not look at the
    // observation: a missing step needs no branch.
    __device__ __forceinline__ void draw_step(const GState<D>& xf, double& x, const double* e, bool& ok) const {
        GState<D> xp = xf;
        double AP[D];
        predict(xp, AP);      // (the filter's own predict, to the bit: both sides of the hand-over check see the same filtering states)
        double Xc[D];
        gain_cols(xp.P, AP, Xc, ok);
        // ---- column j of Z = U G' from the published U (U[i][k] = tile[i + 8 k], k >= i)
        double Z[D];
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_GU for (int k = i; k < D; ++k) acc = fma(tile[i + G * k], Xc[k], acc);
            Z[i] = acc;
        }
        // ---- column j of L = Pf - Z' Z: ONE publication of Z (Z[k][i] = tile[k + 8 i])
        publish(Z);
        double Lc[D];
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = xf.P[i];
            TGP_GU for (int k = 0; k < D; ++k) acc = fma(-tile[k + G * i], Z[k], acc);
            Lc[i] = acc;
        }
        double UL[D], rinvL[D];
        chol_cols(Lc, tgp_sweep::kJitterDraw, UL, rinvL, ok);
        // ---- the mean: x_j = mf_j + nz_j + sum_k G'[k][j] (x+ - mp)_k
        double dm[D];
        gather(x - xp.m, dm, V0);
        double acc = xf.m + mul_Ut(UL, e);
        TGP_GU for (int k = 0; k < D; ++k) acc = fma(Xc[k], dm[k], acc);
        x = act ? acc : 0.0;
    }
    // how far apart two sample states are: the mean part of `distance`, this lane's element, then the group's maximum
    __device__ __forceinline__ double draw_distance(const GroupModelC& mc, double a, double b) const {
        const double worst = act ? ::fabs(a - b) / (mc.sd[j] + ::fabs(a) + ::fabs(b)) : 0.0;
        return group_max(worst);
    }

    // packed state records (checkpoints in HBM, a block's filtering states in LDS): [m d | upper triangle, column by column]
    __device__ __forceinline__ void store_packed(double* q, const GState<D>& x) const {
        if (act) {
            q[j] = x.m;
            TGP_GU for (int i = 0; i < D; ++i)
                if (i <= j) q[D + j * (j + 1) / 2 + i] = x.P[i];
        }
    }
    __device__ __forceinline__ void load_packed(const double* q, GState<D>& x) const {
        x.m = 0.0;
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] = 0.0;
        if (act) {
            x.m = q[j];
            TGP_GU for (int i = 0; i < D; ++i) {
                const int lo = i < j ? i : j, hi = i < j ? j : i;
                x.P[i] = q[D + hi * (hi + 1) / 2 + lo];
            }
        }
    }
    // how far apart two states are, relative to the size of a state (tgp_sweep_body.hpp state_distance): this lane's column, then the group's maximum
    __device__ __forceinline__ double distance(const GroupModelC& mc, const GState<D>& a, const GState<D>& b) const {
        double worst = 0.0;
        if (act) {
            const double sj = mc.sd[j];
            worst = ::fabs(a.m - b.m) / (sj + ::fabs(a.m) + ::fabs(b.m));
            TGP_GU for (int i = 0; i < D; ++i) {
                const double r = ::fabs(a.P[i] - b.P[i]) / (mc.sd[i] * sj);
                worst = r > worst ? r : worst;
            }
        }
        return group_max(worst);
    }
    __device__ __forceinline__ bool finite(const GState<D>& x) const {
        double s = ::fabs(x.m);
        TGP_GU for (int i = 0; i < D; ++i) s += ::fabs(x.P[i]);
        return group_sum(s) < 1e300;      // (false for NaN as well)
    }

    // ---- the adjoint of the filter (k_sweep_group_adjoint): tgp_sweep_body.hpp adjoint_step in the column layout.  An adjoint
    // (l, L) = d logpdf / d (m, P) is held like a state: lane j holds l_j (GState::m) and column j of L (GState::P; L is symmetric).
    // One step backwards.  xf: the filtering state in FRONT of step t; ad: the adjoint behind it on entry, in front of it on return.  A missing step
    // (obs == false; the padded steps behind the series' end are such) passes the adjoint through the predict alone: gh_t = gR_t = 0.
    // ACC: the step's share of the block gradients is added to acc (column j of gA and gQ, element j of ga and gH, the sums of gh_t and gR_t).
    template <bool ACC>
    __device__ __forceinline__ void adjoint_step(const GState<D>& xf, double y, double Rt, double ht, bool obs, GState<D>& ad, GAcc<D>* acc, double& gh_t,
                                                 double& gR_t) const {
        GState<D> xp = xf;
        double AP[D];
        predict(xp, AP);      // (the filter's own predict, to the bit)
        double vj = 0.0;      // V = Pp H, element j
        TGP_GU for (int i = 0; i < D; ++i) vj = fma(xp.P[i], H[i], vj);
        const double s2 = group_sum(Hj * vj) + Rt;
        const double hm = group_sum(Hj * xp.m) + ht;
        const double S = obs ? s2 : 1.0;
        const double iS = obs ? fast_rcp(S) : 0.0;      // (a missing step: every term of the update's adjoint below is a multiple of iS or v)
        const double v = obs ? (y - hm) : 0.0;
        const double viS = v * iS;
        double V[D];
        gather(vj, V, V1);
        double lvj = 0.0;      // (L V)_j = sum_i L[i][j] V_i: lane-local by symmetry
        TGP_GU for (int i = 0; i < D; ++i) lvj = fma(ad.P[i], V[i], lvj);
        const double lV = group_sum(ad.m * vj);
        const double VLV = group_sum(vj * lvj);
        const double vbar = (lV - v) * iS;
        const double Sbar = fma(fma(-lV, v, VLV) * iS, iS, -0.5 * fma(-viS, viS, iS));
        const double vbj = fma(Sbar, Hj, fma(ad.m, viS, -2.0 * iS * lvj));
        gh_t = -vbar;
        gR_t = Sbar;
        double Vb[D];
        gather(vbj, Vb, V0);
        const double mbj = fma(-vbar, Hj, ad.m);
        double Pb[D];      // column j of Pb = L + (Vb H' + H Vb') / 2
        TGP_GU for (int i = 0; i < D; ++i) Pb[i] = fma(0.5, fma(Vb[i], Hj, H[i] * vbj), ad.P[i]);
        if (ACC) {
            double a = fma(Sbar, vj, -vbar * xp.m);
            TGP_GU for (int i = 0; i < D; ++i) a = fma(xp.P[i], Vb[i], a);
            acc->gH += a;
            acc->ga += mbj;
            acc->gh -= vbar;
            acc->gR += Sbar;
            TGP_GU for (int i = 0; i < D; ++i) acc->gQ[i] += Pb[i];
        }
        // Pb and mb through the tile (ONE trip, as predict's): every lane reads the whole of Pb, a wave-wide broadcast per element (rows and columns
        // < D only: a padding lane's column is zero, the rows >= D are never written)
        wave_sync();
        TGP_GU for (int i = 0; i < D; ++i) tile[i + G * j] = Pb[i];
        tile[V0 + j] = mbj;
        wave_sync();
        double mb[D], Ac[D], u[D], w[D];
        TGP_GU for (int k = 0; k < D; ++k) {
            mb[k] = tile[V0 + k];
            Ac[k] = sA[G * k + j];      // column j of A (zero in a padding lane)
        }
        TGP_GU for (int i = 0; i < D; ++i) {
            double au = 0.0, aw = 0.0;
            TGP_GU for (int k = 0; k < D; ++k) {
                const double p = tile[i + G * k];
                if (ACC) au = fma(p, AP[k], au);
                aw = fma(p, Ac[k], aw);
            }
            u[i] = au;
            w[i] = aw;
        }
        if (ACC) { TGP_GU for (int i = 0; i < D; ++i) acc->gA[i] += fma(2.0, u[i], mb[i] * xf.m); }      // gA += mb m' + 2 Pb (A P), column j
        // l <- A' mb;  L <- A' Pb A, column j = A' w
        double al = 0.0;
        TGP_GU for (int k = 0; k < D; ++k) al = fma(Ac[k], mb[k], al);
        ad.m = al;
        TGP_GU for (int i = 0; i < D; ++i) {
            double a = 0.0;
            TGP_GU for (int k = 0; k < D; ++k) a = fma(sA[G * k + i], w[k], a);
            ad.P[i] = a;
        }
    }
    // How far apart two adjoints are (tgp_sweep_body.hpp adjoint_distance): |dl_i| sd_i, |dL_ij| sd_i sd_j, absolute; this lane's column, then the
    // group's maximum.  Compared with mc.tol_b.
    __device__ __forceinline__ double adjoint_distance(const GroupModelC& mc, const GState<D>& a, const GState<D>& b) const {
        double worst = 0.0;
        if (act) {
            const double sj = mc.sd[j];
            worst = ::fabs(a.m - b.m) * sj;
            TGP_GU for (int i = 0; i < D; ++i) {
                const double r = ::fabs(a.P[i] - b.P[i]) * (mc.sd[i] * sj);
                worst = r > worst ? r : worst;      // (a NaN on either side compares false everywhere: caught by the caller's finite test)
            }
        }
        return group_max(worst);
    }
};

// tgp_sweep_group_sde.hip: a call on an SDE-described model -- k_sweep_group_sde<d, XS, post> on nwaves workgroups; ka.st.tau holds the gaps
void launch_sde(int d, unsigned nwaves, hipStream_t stream, const GArgs& ka, const tgp_sweep::GroupSdeC& sc, bool post);

}  // namespace tgp_sweep_group
