// Host half of the sweep engine (tgp_sweep.hpp): the geometry of a call -- chunk length, warm-up lengths -- and the model's shared blocks in the
// form the kernel reads them.  Plain C++ (no HIP): tests/hostsim/sweepsim.cpp builds the same plan on the CPU.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "tgp_sweep_body.hpp"

namespace tgp_sweep {

constexpr int kMaxD = 4;
constexpr int kOwned = 62;           // chunks a wave owns (lanes 1 .. 62)

// Host copies of the model's shared blocks (column-major, as tgp_model_set takes them).
struct ModelHost {
    int d = 0;
    bool sde = false;
    const double* A = nullptr;      // LTI: [d*d];  SDE: the first transition A1
    const double* a = nullptr;      // [d]
    const double* Q = nullptr;      // LTI: [d*d];  SDE: Q1 (checked against Pinf - A1 Pinf A1')
    const double* H = nullptr;      // [d]
    double hh = 0.0, R = 0.0;       // shared values (ignored where a per-step stream is given; R also feeds the warm-up estimate)
    const double* x0m = nullptr;    // [d]
    const double* x0P = nullptr;    // [d*d]  (SDE: also Pinf, unless Pinf is given)
    const double* Pinf = nullptr;   // SDE, optional: [d*d] the stationary covariance of a model whose prior was replaced (tgp_model_set_x0)
    const double* coef = nullptr;   // SDE: [lambda d | N d*d | N^2/2 d*d | ...] as ModelView::sde
    double tau_typ = 0.0;           // SDE: a typical gap (the warm-up estimate)
};

struct Plan {
    int d = 0;
    bool sde = false;
    int C = 0, W = 0, Wb = 0;
    int Wd = 0;                     // the draw's warm-up (k_sweep_draw): steps of a chunk's head the walk is composed over
    int Wa = 0;                     // the adjoint's warm-up (k_sweep_adjoint): steps of a chunk's head the adjoint walks from zero
    int64_t T = 0, nchunks = 0, nwaves = 0;
    double mc[160];                 // the ModelC<d> of the call, as plain doubles (copied into the typed kernel argument)
};
struct Forced {                     // test hook: geometry of the next plan (0: automatic)
    int C = 0, W = 0, Wb = 0;
    int Wd = 0;
    int Wa = 0;
};

namespace plan_detail {

template <int D> inline void fill_model(const ModelHost& m, ModelC<D>& mc) {
    std::memset(&mc, 0, sizeof mc);
    for (int i = 0; i < D * D; ++i) mc.A[i] = m.A[i];
    for (int i = 0; i < D; ++i) {
        mc.a[i] = m.a[i];
        mc.H[i] = m.H[i];
        mc.x0m[i] = m.x0m[i];
    }
    for (int j = 0; j < D; ++j)
        for (int i = 0; i <= j; ++i) {
            mc.Q[pidx(i, j)] = 0.5 * (m.Q[i + j * D] + m.Q[j + i * D]);
            mc.x0P[pidx(i, j)] = m.x0P[i + j * D];      // Symmetric(P): the upper triangle is what the reference reads (lgc.jl:50)
        }
    mc.hh = m.hh;
    mc.R = m.R;
    if (m.sde) {
        const double* q = m.coef;
        for (int i = 0; i < D; ++i) mc.lam[i] = q[i];
        for (int i = 0; i < D * D; ++i) {
            mc.N1[i] = q[D + i];
            mc.N2[i] = q[D + D * D + i];
        }
    }
}

// stationary covariance of x' = A x + w, w ~ N(0, Q): P = A P A' + Q by doubling (spectral radius < 1); false: no such P
template <int D> inline bool lyapunov(const double* A, const double* Q, double* P) {
    double M[D * D], S[D * D], T1[D * D], T2[D * D];
    for (int i = 0; i < D * D; ++i) { M[i] = A[i]; S[i] = Q[i]; }
    for (int it = 0; it < 60; ++it) {
        // S <- S + M S M' ; M <- M M
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k) a += M[i + k * D] * S[k + j * D];
                T1[i + j * D] = a;
            }
        double dmax = 0.0, smax = 0.0;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k) a += T1[i + k * D] * M[j + k * D];
                T2[i + j * D] = a;
                dmax = std::max(dmax, std::fabs(a));
            }
        for (int i = 0; i < D * D; ++i) { S[i] += T2[i]; smax = std::max(smax, std::fabs(S[i])); }
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k) a += M[i + k * D] * M[k + j * D];
                T1[i + j * D] = a;
            }
        for (int i = 0; i < D * D; ++i) M[i] = T1[i];
        if (!std::isfinite(smax) || smax > 1e200) return false;
        if (dmax <= 1e-17 * smax) {
            for (int i = 0; i < D * D; ++i) P[i] = S[i];
            return true;
        }
    }
    return false;
}

// How many steps until a start state is forgotten to `tol`: the closed loop of the stationary filter with every step observed at noise R,
// Phi = A (I - K H'); the number of steps n with max |Phi^n| <= tol (a Jordan block's powers carry a polynomial factor the spectral
// radius does not show: multiply, do not estimate).  0: not within `cap` steps.
template <int D> inline int forget_steps(const double* A, const double* Q, const double* H, double R, double tol, int cap) {
    double P[D * D];
    if (!lyapunov<D>(A, Q, P)) return 0;
    double Phi[D * D];
    for (int it = 0; it < 4096; ++it) {      // Riccati iteration to the stationary PREDICTED covariance
        double V[D], s = R;
        for (int j = 0; j < D; ++j) {
            double a = 0.0;
            for (int k = 0; k < D; ++k) a += H[k] * P[k + j * D];
            V[j] = a;
        }
        for (int k = 0; k < D; ++k) s += V[k] * H[k];
        if (!(s > 0.0)) return 0;
        double Pf[D * D], AP[D * D], Pn[D * D];
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) Pf[i + j * D] = P[i + j * D] - V[i] * V[j] / s;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k) a += A[i + k * D] * Pf[k + j * D];
                AP[i + j * D] = a;
            }
        double ch = 0.0, sc = 0.0;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = Q[i + j * D];
                for (int k = 0; k < D; ++k) a += AP[i + k * D] * A[j + k * D];
                Pn[i + j * D] = a;
                ch = std::max(ch, std::fabs(a - P[i + j * D]));
                sc = std::max(sc, std::fabs(a));
            }
        for (int i = 0; i < D * D; ++i) P[i] = Pn[i];
        if (ch <= 1e-14 * sc || it == 4095) {
            // Phi = A (I - K H'), K = V / s
            for (int j = 0; j < D; ++j)
                for (int i = 0; i < D; ++i) {
                    double a = A[i + j * D];
                    double ak = 0.0;
                    for (int k = 0; k < D; ++k) ak += A[i + k * D] * V[k];
                    a -= ak / s * H[j];
                    Phi[i + j * D] = a;
                }
            break;
        }
    }
    // scale-free powers: in the coordinates of the stationary prior's standard deviations
    double sd[D];
    {
        double Ps[D * D];
        if (!lyapunov<D>(A, Q, Ps)) return 0;
        for (int i = 0; i < D; ++i) sd[i] = std::sqrt(std::max(Ps[i + i * D], 1e-300));
    }
    double M[D * D], Tm[D * D];
    for (int j = 0; j < D; ++j)
        for (int i = 0; i < D; ++i) M[i + j * D] = Phi[i + j * D] * sd[j] / sd[i];
    double Pw[D * D];
    std::memcpy(Pw, M, sizeof Pw);
    for (int n = 1; n <= cap; ++n) {
        double mx = 0.0;
        for (int i = 0; i < D * D; ++i) mx = std::max(mx, std::fabs(Pw[i]));
        if (mx <= tol) return n;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k) a += Pw[i + k * D] * M[k + j * D];
                Tm[i + j * D] = a;
            }
        std::memcpy(Pw, Tm, sizeof Pw);
    }
    return 0;
}

template <int D> inline void host_sde_A(const double* q, double tau, double* A) {
    for (int j = 0; j < D; ++j)
        for (int i = 0; i < D; ++i)
            A[i + j * D] = std::exp(-q[i] * tau) * (tau * tau * q[D + D * D + i + j * D] + tau * q[D + i + j * D] + (i == j ? 1.0 : 0.0));
}

// What a handed-over state may be off by, relative to the size of a state.  Forwards 1e-12: the log marginal likelihood is held to 1e-10 relative
// and the innovations behind a hand-over inherit its error.  Backwards 1e-11: the marginals are held to 1e-8 of their scale.
constexpr double kTol = 1e-12, kTolBack = 1e-11;
constexpr int kMaxWarm = 4096;

// The stationary prior of an LTI model (where a warm-up starts from): Aty / Qty = the transition with Q symmetrised, gm the stationary mean, Ps the
// stationary covariance.  false: the transition has none.
template <int D> inline bool stationary_prior(const ModelHost& m, double* Aty, double* Qty, double* gm, double* Ps) {
    for (int i = 0; i < D * D; ++i) { Aty[i] = m.A[i]; Qty[i] = 0.5 * (m.Q[i] + m.Q[(i % D) * D + i / D]); }
    if (!lyapunov<D>(Aty, Qty, Ps)) return false;
    // stationary mean: (I - A) gm = a, by fixed-point iteration (spectral radius < 1)
    for (int i = 0; i < D; ++i) gm[i] = 0.0;
    for (int it = 0; it < 100000; ++it) {
        double nx[D], ch = 0.0;
        for (int i = 0; i < D; ++i) {
            double acc = m.a[i];
            for (int k = 0; k < D; ++k) acc += Aty[i + k * D] * gm[k];
            nx[i] = acc;
            ch = std::max(ch, std::fabs(acc - gm[i]));
        }
        std::memcpy(gm, nx, sizeof nx);
        if (ch == 0.0 || ch < 1e-300) break;
        double mx = 0.0;
        for (int i = 0; i < D; ++i) mx = std::max(mx, std::fabs(gm[i]));
        if (ch <= 1e-15 * mx) break;
    }
    return true;
}

// The warm-up lengths (multiples of 8) where the caller has none (W / Wb <= 0 on entry): the forgetting-rate estimate with its margin.
// false: the filter does not forget within kMaxWarm steps.
template <int D> inline bool estimate_warmups(const double* Aty, const double* Qty, const double* H, double R, int& W, int& Wb, std::string* why) {
    if (W <= 0 || Wb <= 0) {
        // (the estimate is for a series observed at every step with the representative noise: missing steps and larger noise slow the forgetting
        //  -- hence the margin -- and the checks decide: a call that finds its warm-ups short is repeated with longer ones and the bound model
        //  remembers them.  Measured at the bench model with 10 % missing: 1e-12 forwards needs 100 steps, the estimate says 96 + margin.)
        const double Rrep = R > 0.0 && R < 1e14 ? R : 1.0;
        const int nf = forget_steps<D>(Aty, Qty, H, Rrep, kTol, kMaxWarm);
        const int nb = forget_steps<D>(Aty, Qty, H, Rrep, kTolBack, kMaxWarm);
        if (nf == 0 || nb == 0) {
            if (why) *why = "the filter does not forget a state within 4096 steps";
            return false;
        }
        if (W <= 0) W = nf + nf / 8 + 8;
        if (Wb <= 0) Wb = nb + nb / 8 + 8;
    }
    W = (W + 7) / 8 * 8;
    Wb = (Wb + 7) / 8 * 8;
    return true;
}

template <int D> inline bool plan_d(Plan* e, const Forced& f, const ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, std::string* why, int wd_hint,
                                        int wa_hint) {
    constexpr int B = Geo<D>::B;
    ModelC<D> mc;
    fill_model<D>(m, mc);
    mc.tol = kTol;
    mc.tol_b = kTolBack;
    double Aty[D * D], Qty[D * D];      // a typical step's transition (the warm-up estimate)
    if (m.sde) {
        // the warm-up starts from Pinf (x0P where none is given); the first transition must be consistent with it (Q1 = Pinf - A1 Pinf A1')
        const double* Ps = m.Pinf ? m.Pinf : m.x0P;
        double Pinf[D * D];
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) Pinf[i + j * D] = 0.5 * (Ps[i + j * D] + Ps[j + i * D]);
        double worst = 0.0, scale = 0.0;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k)
                    for (int l = 0; l < D; ++l) a += m.A[i + k * D] * Pinf[k + l * D] * m.A[j + l * D];
                worst = std::max(worst, std::fabs(Pinf[i + j * D] - a - m.Q[i + j * D]));
                scale = std::max(scale, std::fabs(Pinf[i + j * D]));
            }
        if (!(worst <= 1e-11 * scale)) {
            if (why) *why = "first transition not of the form Q1 = Pinf - A1 Pinf A1'";
            return false;
        }
        for (int i = 0; i < D; ++i) mc.gm[i] = m.x0m[i];
        for (int j = 0; j < D; ++j)
            for (int i = 0; i <= j; ++i) mc.gP[pidx(i, j)] = Pinf[i + j * D];
        host_sde_A<D>(m.coef, m.tau_typ, Aty);
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k)
                    for (int l = 0; l < D; ++l) a += Aty[i + k * D] * Pinf[k + l * D] * Aty[j + l * D];
                Qty[i + j * D] = Pinf[i + j * D] - a;
            }
    } else {
        double gm[D], Ps[D * D];
        if (!stationary_prior<D>(m, Aty, Qty, gm, Ps)) {
            if (why) *why = "the transition has no stationary covariance";
            return false;
        }
        for (int i = 0; i < D; ++i) mc.gm[i] = gm[i];
        for (int j = 0; j < D; ++j)
            for (int i = 0; i <= j; ++i) mc.gP[pidx(i, j)] = 0.5 * (Ps[i + j * D] + Ps[j + i * D]);
    }
    int W = w_hint, Wb = wb_hint;
    if (!estimate_warmups<D>(Aty, Qty, m.H, m.R, W, Wb, why)) return false;
    auto up = [](int v, int q) { return (v + q - 1) / q * q; };
    // chunk length: the machine holds 4 waves per CU (their LDS), every wave 62 chunks of its own; a chunk holds the backward warm-up
    const int64_t slots = (int64_t)std::max(num_cu, 1) * 4 * kOwned;
    int64_t C = up((int)std::min<int64_t>((T + slots - 1) / slots, 1 << 20), 8);
    C = std::max<int64_t>(C, 64);
    C = std::max<int64_t>(C, Wb);
    // the draw's warm-up: the backward warm-up's value is the first guess (the walk forgets through the same gains); a draw call that found it short
    // passes a longer one, and the chunk holds it
    int Wd = wd_hint > 0 ? up(wd_hint, 8) : Wb;
    if (wd_hint > 0) C = std::max<int64_t>(C, Wd);
    // the adjoint's warm-up: the forward warm-up's value is the first guess (the adjoint recursion runs through the transposed closed loop of the filter
    // and forgets at its rate); a call that found it short passes a longer one, and the chunk holds it
    int Wa = wa_hint > 0 ? up(wa_hint, 8) : W;
    if (wa_hint > 0) C = std::max<int64_t>(C, Wa);
    if (f.C > 0) C = up(f.C, 8);
    if (f.W > 0) W = up(f.W, 8);
    if (f.Wb > 0) Wb = up(f.Wb, 8);
    if (f.Wd > 0) Wd = up(f.Wd, 8);
    if (f.Wa > 0) Wa = up(f.Wa, 8);
    else if (wa_hint <= 0) Wa = up(W, 8);      // (the first guess follows a forced forward warm-up)
    if (Wb > C) Wb = (int)C;
    if (Wd > C) Wd = (int)C;
    if (Wa > C) Wa = (int)C;
    if (W > kMaxWarm || (f.C == 0 && W > 4 * C)) {
        if (why) *why = "forward warm-up longer than four chunks";
        return false;
    }
    (void)B;
    e->d = D;
    e->sde = m.sde;
    e->T = T;
    e->C = (int)C;
    e->W = W;
    e->Wb = Wb;
    e->Wd = Wd;
    e->Wa = Wa;
    e->nchunks = (T + C - 1) / C;
    e->nwaves = (e->nchunks + kOwned - 1) / kOwned;
    static_assert(sizeof(ModelC<D>) <= sizeof(e->mc), "Plan::mc too small");
    std::memcpy(e->mc, &mc, sizeof mc);
    return true;
}

}  // namespace plan_detail

// Chooses the geometry (chunk length, warm-ups) for this model and series; false: the engine declines (`why` says so).
// w_hint / wb_hint: warm-ups a previous call on the same bound model needed (0: estimate from the model); wd_hint / wa_hint: the same for the draw's and
// the adjoint's warm-ups.
inline bool make_plan(Plan* p, const Forced& f, const ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, std::string* why, int wd_hint = 0,
                      int wa_hint = 0) {
    if (m.d < 1 || m.d > kMaxD || T < 1) {
        if (why) *why = "state dimension";
        return false;
    }
    switch (m.d) {
        case 1: return plan_detail::plan_d<1>(p, f, m, T, w_hint, wb_hint, num_cu, why, wd_hint, wa_hint);
        case 2: return plan_detail::plan_d<2>(p, f, m, T, w_hint, wb_hint, num_cu, why, wd_hint, wa_hint);
        case 3: return plan_detail::plan_d<3>(p, f, m, T, w_hint, wb_hint, num_cu, why, wd_hint, wa_hint);
        default: return plan_detail::plan_d<4>(p, f, m, T, w_hint, wb_hint, num_cu, why, wd_hint, wa_hint);
    }
}

// ---- the group sweep (tgp_sweep_group.hip): the same algorithm at 5 <= d <= 8, a chunk spread over 8 lanes ---------------------------
// A wave holds 8 groups = 8 consecutive chunks.  Group 0 only warms up for group 1; in a posterior call group 7 only warms up (backwards) for group 6.
// Both forms of a model: LTI (k_sweep_group) and SDE-described on irregular inputs (k_sweep_group_sde).
constexpr int kGroupMinD = 5, kGroupMaxD = 8;
constexpr int kGroupLanes = 8, kGroupsPerWave = 8;
// waves resident per CU: two per SIMD by LDS and registers, but one where the posterior kernel takes more than 256 registers (d >= 6:
// profiles/sweep_group_resources.txt) -- the grid is sized for what is resident, one round of waves
constexpr int group_waves_per_cu(int d, bool post) { return (post && d >= 6) ? 4 : 8; }
constexpr int64_t kGroupMinT = 2048;           // shorter series stay on the general engine
constexpr int group_owned(bool post) { return post ? kGroupsPerWave - 2 : kGroupsPerWave - 1; }
// steps per checkpoint block: the block's filtering states (d + d (d + 1) / 2 doubles per step and group) sit in LDS during the backward run
constexpr int group_block(int d) { return d <= 6 ? 8 : 4; }
// The adjoint call (k_sweep_group_adjoint) runs in the posterior call's geometry.  Doubles a wave leaves behind its 4 status words: gA d*d, ga d,
// gQ packed, gH d, the sums of gh_t and gR_t, gx0m d, gx0P packed (the lane sweep's record).
constexpr int group_adjoint_sums(int d) { return d * d + d + d * (d + 1) / 2 + d + 2 + d + d * (d + 1) / 2; }
// waves resident per CU in an adjoint call, from the kernel's register counts as group_waves_per_cu's (profiles/sweep_group_adjoint_resources.txt):
// 8 where it takes at most 256 registers (d = 5, 6: 220 .. 254), else 4 (d = 7, 8: 262 .. 290)
constexpr int group_adjoint_waves_per_cu(int d) { return d <= 6 ? 8 : 4; }
// waves resident per CU in a draw call (k_sweep_group_draw), from the kernel's register counts in the same way
// (profiles/sweep_group_draw_resources.txt): 8 at d = 5 (237 .. 244 registers), else 4 (d = 6, 7, 8: 277 .. 412)
constexpr int group_draw_waves_per_cu(int d) { return d <= 5 ? 8 : 4; }
// waves resident per CU in a call on an SDE-described model (k_sweep_group_sde), from the kernel's register counts in the same way
// (profiles/sweep_group_sde_resources.txt has the counts and tests/test_sweep_group_sde_resources.py holds this function to them): today every logpdf
// kernel is within 256 registers and every posterior kernel above, whatever d
constexpr int group_sde_waves_per_cu(int d, bool post) { return (void)d, post ? 4 : 8; }

// The steps [t0, t1) of group g (0 .. 7) of a wave, as the kernel and the tests compute them: the wave's groups hold the chunks
// wave * owned - 1 .. wave * owned + 6.  runs: the group runs its chunk (group 0 only warms up); owned: it writes output and sums.
struct GroupSpan {
    long long t0, t1;
    bool runs, owned;
};
TGP_HD GroupSpan group_span(long long wave, int g, int owned, long long nchunks, int C, long long T) {
    const long long c = wave * owned + g - 1;
    const bool active = c >= 0 && c < nchunks;
    GroupSpan s;
    s.t0 = active ? c * C : 0;
    s.t1 = active ? s.t0 + C : 0;
    s.t1 = s.t1 < T ? s.t1 : (active ? T : 0);
    s.runs = active && g >= 1;
    s.owned = s.runs && g <= owned;
    return s;
}

// The model's shared blocks as the group kernels read them: padded to 8 whatever d is (the padding is zero), A row-major (read from LDS as a
// broadcast), the symmetric blocks full and column-major (lane j reads column j).
struct GroupModelC {
    double A[64];                     // [8 i + k]
    double a[8], H[8], x0m[8], gm[8];
    double Q[64], x0P[64], gP[64];    // [i + 8 j]
    double sd[8];                     // sqrt(gP[i][i]): the scale of a state's element i (the hand-over checks)
    double hh, R, tol, tol_b;
};

// What an SDE-described model adds (k_sweep_group_sde): exp(F tau) = diag(e^(-lam tau)) (I + tau N1 + tau^2 N2) per block (ModelView::sde),
// padded to 8 and row-major like GroupModelC::A.  The blocks of the closed form are contiguous and at most 3 wide (tgp_api.hip sde_closed_form), so
// N1 and N2 are zero outside the band |i - k| <= 2, which is all the kernel multiplies (the plan checks it).  GroupModelC carries the rest: gP = Pinf,
// (x0m, x0P) = the prior predicted through the first transition (the state in FRONT of update 0), A and Q unused.
struct GroupSdeC {
    double lam[8];
    double N1[64], N2[64];      // [8 i + k]
};
constexpr int kGroupSdeBand = 2;

struct GroupPlan {
    bool sde = false;          // an SDE-described model: k_sweep_group_sde reads mc and sc
    GroupSdeC sc;
    int d = 0, B = 0, owned = 0;
    bool post = false;
    int C = 0, W = 0, Wb = 0;
    int64_t T = 0, nchunks = 0, nwaves = 0;
    GroupModelC mc;
    bool adjoint = false;      // an adjoint call: post's geometry, Wb holds the adjoint's warm-up Wa
    bool draw = false;         // a draw call: post's geometry, Wb holds the draw's warm-up Wd
};

namespace plan_detail {

template <int D> inline bool plan_group_d(GroupPlan* e, const Forced& f, const ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, bool post,
                                          std::string* why, bool adjoint = false, bool draw = false) {
    double Aty[D * D], Qty[D * D], gm[D], Ps[D * D];
    double p0m[D], p0P[D * D];      // SDE: the prior predicted through the first transition
    if (m.sde) {
        // plan_d's SDE branch: the warm-up starts from (x0m, Pinf) (x0P where no Pinf is given); the first transition must be consistent with it
        const double* Pg = m.Pinf ? m.Pinf : m.x0P;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) Ps[i + j * D] = 0.5 * (Pg[i + j * D] + Pg[j + i * D]);
        double worst = 0.0, scale = 0.0;
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k)
                    for (int l = 0; l < D; ++l) a += m.A[i + k * D] * Ps[k + l * D] * m.A[j + l * D];
                worst = std::max(worst, std::fabs(Ps[i + j * D] - a - m.Q[i + j * D]));
                scale = std::max(scale, std::fabs(Ps[i + j * D]));
            }
        if (!(worst <= 1e-11 * scale)) {
            if (why) *why = "first transition not of the form Q1 = Pinf - A1 Pinf A1'";
            return false;
        }
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i)
                if (std::abs(i - j) > kGroupSdeBand && (m.coef[D + i + j * D] != 0.0 || m.coef[D + D * D + i + j * D] != 0.0)) {
                    if (why) *why = "closed form wider than the band the kernel multiplies";
                    return false;
                }
        for (int i = 0; i < D; ++i) gm[i] = m.x0m[i];
        host_sde_A<D>(m.coef, m.tau_typ, Aty);
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.0;
                for (int k = 0; k < D; ++k)
                    for (int l = 0; l < D; ++l) a += Aty[i + k * D] * Ps[k + l * D] * Aty[j + l * D];
                Qty[i + j * D] = Ps[i + j * D] - a;
            }
        // step 0 on the host (A1 is not exp(F tau) of any tau once a term is stretched): m <- A1 x0m + a, P <- A1 Symmetric(x0P) A1' + Q1; the kernel
        // keeps this state at t == 0 instead of predicting
        for (int i = 0; i < D; ++i) {
            double a = m.a[i];
            for (int k = 0; k < D; ++k) a += m.A[i + k * D] * m.x0m[k];
            p0m[i] = a;
        }
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < D; ++i) {
                double a = 0.5 * (m.Q[i + j * D] + m.Q[j + i * D]);
                for (int k = 0; k < D; ++k)
                    for (int l = 0; l < D; ++l) a += m.A[i + k * D] * m.x0P[std::min(k, l) + std::max(k, l) * D] * m.A[j + l * D];
                p0P[i + j * D] = a;
            }
        for (int j = 0; j < D; ++j)
            for (int i = 0; i < j; ++i) p0P[i + j * D] = p0P[j + i * D] = 0.5 * (p0P[i + j * D] + p0P[j + i * D]);
    } else if (!stationary_prior<D>(m, Aty, Qty, gm, Ps)) {
        if (why) *why = "the transition has no stationary covariance";
        return false;
    }
    int W = w_hint, Wb = wb_hint;
    if (!estimate_warmups<D>(Aty, Qty, m.H, m.R, W, Wb, why)) return false;
    // the adjoint's warm-up: the forward warm-up's value is the first guess (plan_d: the adjoint forgets at the filter's rate); a call that found it
    // short passes a longer one
    if (adjoint && wb_hint <= 0) Wb = W;
    // (the draw's warm-up: the backward warm-up's estimate is the first guess, as plan_d's -- the walk forgets through the same gains)
    auto up = [](int v, int q) { return (v + q - 1) / q * q; };
    // chunk length: group_waves_per_cu waves per CU, every wave `owned` chunks of its own; a chunk holds the backward warm-up.  A multiple of 8 (the rows
    // of the observation stream), hence of the checkpoint block.
    const int owned = group_owned(post);
    const int per_cu = m.sde ? group_sde_waves_per_cu(D, post) : adjoint ? group_adjoint_waves_per_cu(D) : draw ? group_draw_waves_per_cu(D) : group_waves_per_cu(D, post);
    const int64_t slots = (int64_t)std::max(num_cu, 1) * per_cu * owned;
    int64_t C = up((int)std::min<int64_t>((T + slots - 1) / slots, 1 << 20), 8);
    C = std::max<int64_t>(C, 64);
    C = std::max<int64_t>(C, Wb);
    if (f.C > 0) C = up(f.C, 8);
    if (f.W > 0) W = up(f.W, 8);
    if (f.Wb > 0) Wb = up(f.Wb, 8);
    else if (adjoint && wb_hint <= 0) Wb = W;      // (the first guess follows a forced forward warm-up)
    if (Wb > C) Wb = (int)C;
    if (W > kMaxWarm || (f.C == 0 && W > 4 * C)) {
        if (why) *why = "forward warm-up longer than four chunks";
        return false;
    }
    const int64_t nchunks = (T + C - 1) / C;
    if (nchunks < owned) {
        if (why) *why = "fewer chunks than one wave owns";
        return false;
    }
    e->d = D;
    e->B = group_block(D);
    e->owned = owned;
    e->post = post;
    e->adjoint = adjoint;
    e->draw = draw;
    e->T = T;
    e->C = (int)C;
    e->W = W;
    e->Wb = Wb;
    e->nchunks = nchunks;
    e->nwaves = (nchunks + owned - 1) / owned;
    GroupModelC& mc = e->mc;
    std::memset(&mc, 0, sizeof mc);
    for (int i = 0; i < D; ++i) {
        mc.a[i] = m.a[i];
        mc.H[i] = m.H[i];
        mc.x0m[i] = m.x0m[i];
        mc.gm[i] = gm[i];
        for (int k = 0; k < D; ++k) mc.A[8 * i + k] = m.A[i + k * D];
    }
    for (int j = 0; j < D; ++j)
        for (int i = 0; i < D; ++i) {
            const int lo = std::min(i, j), hi = std::max(i, j);
            mc.Q[i + 8 * j] = Qty[i + j * D];
            mc.x0P[i + 8 * j] = m.x0P[lo + hi * D];      // Symmetric(P): the upper triangle is what the reference reads (lgc.jl:50)
            mc.gP[i + 8 * j] = 0.5 * (Ps[i + j * D] + Ps[j + i * D]);
        }
    for (int i = 0; i < D; ++i) mc.sd[i] = std::sqrt(mc.gP[i + 8 * i]);
    mc.hh = m.hh;
    mc.R = m.R;
    mc.tol = kTol;
    mc.tol_b = kTolBack;
    e->sde = m.sde;
    std::memset(&e->sc, 0, sizeof e->sc);
    if (m.sde) {
        std::memset(mc.A, 0, sizeof mc.A);
        std::memset(mc.Q, 0, sizeof mc.Q);
        for (int i = 0; i < D; ++i) {
            mc.x0m[i] = p0m[i];
            e->sc.lam[i] = m.coef[i];
            for (int k = 0; k < D; ++k) {
                mc.x0P[i + 8 * k] = p0P[i + k * D];
                e->sc.N1[8 * i + k] = m.coef[D + i + k * D];
                e->sc.N2[8 * i + k] = m.coef[D + D * D + i + k * D];
            }
        }
    }
    return true;
}

}  // namespace plan_detail

// The geometry of a group-sweep call (LTI form, or SDE-described: m.sde); false: the engine declines (`why` says so).  post: a posterior call (6 of a wave's 8 groups own
// output instead of 7).  w_hint / wb_hint as make_plan's.  adjoint (with post): an adjoint call -- the backward slot carries the adjoint's warm-up Wa
// (wb_hint: a Wa that a previous call needed, 0: the forward warm-up's value; a forced Wb forces Wa).  draw (with post): a draw call
// (k_sweep_group_draw) -- the backward slot carries the draw's warm-up Wd (wb_hint: a Wd that a previous call needed, 0: the backward
// warm-up's estimate; a forced Wb forces Wd; the chunk grows to hold it).
inline bool plan_group(GroupPlan* p, const Forced& f, const ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, bool post, std::string* why,
                       bool adjoint = false, bool draw = false) {
    if (m.d < kGroupMinD || m.d > kGroupMaxD) {
        if (why) *why = "state dimension";
        return false;
    }
    if (m.sde && (adjoint || draw)) {      // (the gradient and the draw of an SDE-described model at these d: the general engine)
        if (why) *why = "SDE-described model";
        return false;
    }
    if (T < kGroupMinT) {
        if (why) *why = "series shorter than 2048 steps";
        return false;
    }
    switch (m.d) {
        case 5: return plan_detail::plan_group_d<5>(p, f, m, T, w_hint, wb_hint, num_cu, post, why, adjoint, draw);
        case 6: return plan_detail::plan_group_d<6>(p, f, m, T, w_hint, wb_hint, num_cu, post, why, adjoint, draw);
        case 7: return plan_detail::plan_group_d<7>(p, f, m, T, w_hint, wb_hint, num_cu, post, why, adjoint, draw);
        default: return plan_detail::plan_group_d<8>(p, f, m, T, w_hint, wb_hint, num_cu, post, why, adjoint, draw);
    }
}

}  // namespace tgp_sweep
