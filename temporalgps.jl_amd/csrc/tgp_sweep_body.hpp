// Per-lane arithmetic of the sweep engine (tgp_sweep.hip): the reference's sequential recursions for ONE chunk of consecutive
// steps with time-varying gains -- a missing-data mask, a noise variance per step, irregular spacing -- on a state (m, packed upper P) in
// registers.  Host- and device-callable: tests/hostsim runs the very same functions lane by lane on the CPU (tests/test_sweep_host.py).
//
// Reference semantics restated here (file:line under /root/reference/src):
//   predict              models/linear_gaussian_conditionals.jl:46-52     (A Symmetric(P)) A' + Q  (upper triangle kept)
//   posterior_and_lml    models/linear_gaussian_conditionals.jl:247-257   ScalarOutputLGC; a missing step is skipped (missings.jl:8-23:
//                        y := 0, R := 1e15 and the compensated volume term agree with skipping to ~1e-15 relative)
//   invert_dynamics      models/lgssm.jl:231-238                           G = Pf A' (Pp + 1e-10 I)^-1 by Cholesky, as there
//   step_marginals       models/lgssm.jl:111-115 (Reverse)                 x <- G x + g, P <- G P G' + L, in gain form:
//                        ms = mf + G (ms+ - mp),  Ps = Pf + G (Ps+ - Pp - 1e-10 I) G'   (L = Pf - G (Pp + 1e-10 I) G' substituted)
//   broadcast_components gp/lti_sde.jl:135-146                             A_k = exp(F tau_k) in closed form per Matern block;
//                        Q_k = Pinf - A_k Pinf A_k' is never formed: A P A' + Q_k = A (P - Pinf) A' + Pinf
#pragma once
#include "tgp_math.hpp"

namespace tgp_sweep {

constexpr double kJitter = 1e-10;      // lgssm.jl:235
constexpr double kLog2Pi = 1.8378770664093454835606594728112;

template <int D> struct SD {
    static constexpr int DD = D * D, DS = D * (D + 1) / 2, NS = D + DS;
};
// packed upper triangle, column by column (tgp_math_body.inc store_sym): entry (i, j), i <= j, sits at j (j + 1) / 2 + i
TGP_HD constexpr int pidx(int i, int j) { return i <= j ? j * (j + 1) / 2 + i : i * (i + 1) / 2 + j; }

// 1 / x and (sqrt x, 1 / sqrt x) from the hardware's approximate v_rcp_f64 / v_rsq_f64 and two Newton (Goldschmidt) steps each: ~1 ulp,
// 5 / 8 instructions instead of the 12 / 25 of an IEEE division / sqrt + division (the passes are bound by their instruction stream).
TGP_HD double fast_rcp(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
    double r = __builtin_amdgcn_rcp(x);
    double e = ::fma(-x, r, 1.0);
    r = ::fma(r, e, r);
    e = ::fma(-x, r, 1.0);
    r = ::fma(r, e, r);
    return r;
#else
    return 1.0 / x;
#endif
}
TGP_HD void fast_sqrt_rsqrt(double x, double& s, double& rs) {
#if defined(__HIP_DEVICE_COMPILE__)
    const double r0 = __builtin_amdgcn_rsq(x);
    double g = x * r0, hh = 0.5 * r0;
    double e = ::fma(-hh, g, 0.5);
    g = ::fma(g, e, g);
    hh = ::fma(hh, e, hh);
    e = ::fma(-hh, g, 0.5);
    g = ::fma(g, e, g);
    hh = ::fma(hh, e, hh);
    s = g;
    rs = hh + hh;
#else
    s = ::sqrt(x);
    rs = 1.0 / s;
#endif
}

// ---- the model's shared blocks, as the kernel reads them from its argument segment (scalar loads) ----------------------------------
template <int D> struct ModelC {
    double A[D * D], a[D], Q[SD<D>::DS];      // LTI transition.  SDE: A = A1, the series' FIRST transition (lti_sde.jl:139; its Q1 must be
                                              // Pinf - A1 Pinf A1', which the host checks), Q unused
    double H[D];
    double x0m[D], x0P[SD<D>::DS];            // the prior of the series
    double gm[D], gP[SD<D>::DS];              // where a warm-up starts from: the stationary prior (SDE: Pinf)
    double lam[D], N1[D * D], N2[D * D];      // SDE: exp(F tau) = e^(-lam tau) (I + tau N1 + tau^2 N2) per block (ModelView::sde)
    double hh, R;                             // shared emission offset / noise variance (used where no per-step stream is given)
    double tol, tol_b;                        // relative size of a forgotten start state: the checks of the forward / backward hand-overs
};

template <int D> struct State {
    double m[D];
    double P[SD<D>::DS];
};

template <int D> TGP_HD void set_state(State<D>& x, const double* m, const double* P) {
    TGP_UNROLL for (int i = 0; i < D; ++i) x.m[i] = m[i];
    TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) x.P[i] = P[i];
}

// A = exp(F tau) in closed form (tgp_chunk.hpp sde_transition_impl, without its Q)
template <int D> TGP_HD void sde_A(const ModelC<D>& mc, double tau, double* A) {
    double e[D];
    e[0] = ::exp(-mc.lam[0] * tau);
    TGP_UNROLL for (int i = 1; i < D; ++i) e[i] = (mc.lam[i] == mc.lam[i - 1]) ? e[i - 1] : ::exp(-mc.lam[i] * tau);     // (wave-uniform: one exp per block)
    const double t2 = tau * tau;
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) A[i + j * D] = e[i] * ::fma(t2, mc.N2[i + j * D], ::fma(tau, mc.N1[i + j * D], i == j ? 1.0 : 0.0));
}

// AX = A Symmetric(X) (full d x d), X packed
template <int D> TGP_HD void mul_A_sym(const double* A, const double* X, double* AX) {
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(A[i + k * D], X[pidx(k, j)], acc);
            AX[i + j * D] = acc;
        }
}
// out (packed upper) = AX A' + C (packed)
template <int D> TGP_HD void mul_AXAt_plus(const double* AX, const double* A, const double* C, double* out) {
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            double acc = C[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(AX[i + k * D], A[j + k * D], acc);
            out[pidx(i, j)] = acc;
        }
}

// The transition of one step, in the form the predict needs: LTI -> (A, a, Q) of the model; SDE -> A from tau, covariance through Pinf.
template <int D, bool SDE> struct Trans {
    double A[D * D];
    TGP_HD void set(const ModelC<D>& mc, double tau, bool first) {
        if constexpr (SDE) {
            sde_A<D>(mc, first ? 0.0 : tau, A);
            TGP_UNROLL for (int i = 0; i < D * D; ++i) A[i] = first ? mc.A[i] : A[i];
        } else {
            TGP_UNROLL for (int i = 0; i < D * D; ++i) A[i] = mc.A[i];
        }
    }
};

// predict (lgc.jl:46-52).
// AP_out (optional, full d x d): A Symmetric(P) of the INCOMING covariance -- what invert_dynamics multiplies again (lgssm.jl:234).
template <int D, bool SDE> TGP_HD void predict(const ModelC<D>& mc, const double* A, double* m, double* P, double* AP_out = nullptr) {
    double mp[D];
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = mc.a[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(A[i + k * D], m[k], acc);
        mp[i] = acc;
    }
    TGP_UNROLL for (int i = 0; i < D; ++i) m[i] = mp[i];
    double AX[D * D], Pn[SD<D>::DS];
    if constexpr (SDE) {
        if (AP_out) {      // A P and A Pinf separately: the smoother needs A P itself
            double AG[D * D];
            mul_A_sym<D>(A, P, AP_out);
            mul_A_sym<D>(A, mc.gP, AG);
            TGP_UNROLL for (int i = 0; i < D * D; ++i) AX[i] = AP_out[i] - AG[i];
        } else {
            double Dm[SD<D>::DS];
            TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) Dm[i] = P[i] - mc.gP[i];
            mul_A_sym<D>(A, Dm, AX);
        }
        mul_AXAt_plus<D>(AX, A, mc.gP, Pn);
    } else {
        mul_A_sym<D>(A, P, AX);
        if (AP_out) { TGP_UNROLL for (int i = 0; i < D * D; ++i) AP_out[i] = AX[i]; }
        mul_AXAt_plus<D>(AX, A, mc.Q, Pn);
    }
    TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) P[i] = Pn[i];
}

// The log marginal likelihood's running sums of one lane: sum of r^2 / S, the product of the S of up to eight steps (ONE log per eight
// steps: log prod = sum log to rounding), the observed steps.
struct LmlAcc {
    double q = 0.0, logs = 0.0, prod = 1.0, n = 0.0;
    TGP_HD void flush() {
        logs += ::log(prod);
        prod = 1.0;
    }
    TGP_HD double total() const { return -0.5 * (n * kLog2Pi + logs + q); }
};

// posterior_and_lml of a ScalarOutputLGC (lgc.jl:247-257); obs == false: the step is missing, nothing changes.
template <int D> TGP_HD void update(const double* H, double hh, double R, double y, bool obs, double* m, double* P, LmlAcc* acc, bool& ok) {
    double V[D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        double a = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(H[k], P[pidx(k, j)], a);
        V[j] = a;
    }
    double s2 = R, hm = hh;
    TGP_UNROLL for (int k = 0; k < D; ++k) {
        s2 = ::fma(V[k], H[k], s2);
        hm = ::fma(H[k], m[k], hm);
    }
    const double S = obs ? s2 : 1.0;
    ok = ok && (S > 0.0);
    const double iS = obs ? fast_rcp(S) : 0.0;
    const double v = obs ? (y - hm) : 0.0;
    const double viS = v * iS;
    TGP_UNROLL for (int i = 0; i < D; ++i) m[i] = ::fma(V[i], viS, m[i]);
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        const double w = V[j] * iS;
        TGP_UNROLL for (int i = 0; i <= j; ++i) P[pidx(i, j)] = ::fma(-V[i], w, P[pidx(i, j)]);
    }
    if (acc) {
        acc->q = ::fma(v, viS, acc->q);
        acc->prod *= S;
        acc->n += obs ? 1.0 : 0.0;
    }
}

// One step of the reverse-time recursion (lgssm.jl:231-238 + :111-115): xf = filtering state of step t, A = transition of step t + 1,
// xs = smoothing state of step t + 1 on entry, of step t on return.
template <int D, bool SDE> TGP_HD void smooth_step(const ModelC<D>& mc, const double* A, const State<D>& xf, State<D>& xs, bool& ok) {
    constexpr int DS = SD<D>::DS;
    double mp[D], Pp[DS], AP[D * D];
    TGP_UNROLL for (int i = 0; i < D; ++i) mp[i] = xf.m[i];
    TGP_UNROLL for (int i = 0; i < DS; ++i) Pp[i] = xf.P[i];
    predict<D, SDE>(mc, A, mp, Pp, AP);
    // upper Cholesky factor of Pp + jitter I (rows of U, reciprocal pivots)
    double U[D * D], inv[D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < j; ++i) {
            double acc = Pp[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], U[k + j * D], acc);
            U[i + j * D] = acc * inv[i];
        }
        double acc = Pp[pidx(j, j)] + kJitter;
        TGP_UNROLL for (int k = 0; k < j; ++k) acc = ::fma(-U[k + j * D], U[k + j * D], acc);
        ok = ok && (acc > 0.0);
        double s, rs;
        fast_sqrt_rsqrt(acc, s, rs);
        U[j + j * D] = s;
        inv[j] = rs;
    }
    // W = (Pp + jitter I)^-1 (A Pf) = G'   (column j of W: U' z = AP[:, j], U w = z)
    double W[D * D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = AP[i + j * D];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], W[k + j * D], acc);
            W[i + j * D] = acc * inv[i];
        }
        TGP_UNROLL for (int i = D - 1; i >= 0; --i) {
            double acc = W[i + j * D];
            TGP_UNROLL for (int k = i + 1; k < D; ++k) acc = ::fma(-U[i + k * D], W[k + j * D], acc);
            W[i + j * D] = acc * inv[i];
        }
    }
    // gain form: ms = mf + G (ms+ - mp);  Ps = Pf + G (Ps+ - Pp - jitter I) G'     (G[i][k] = W[k + i D])
    double dm[D], Dm[DS];
    TGP_UNROLL for (int i = 0; i < D; ++i) dm[i] = xs.m[i] - mp[i];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) Dm[pidx(i, j)] = xs.P[pidx(i, j)] - Pp[pidx(i, j)] - (i == j ? kJitter : 0.0);
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = xf.m[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(W[k + i * D], dm[k], acc);
        xs.m[i] = acc;
    }
    double GD[D * D];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(W[k + i * D], Dm[pidx(k, j)], acc);
            GD[i + j * D] = acc;
        }
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            double acc = xf.P[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(GD[i + k * D], W[k + j * D], acc);
            xs.P[pidx(i, j)] = acc;
        }
}

// emission predict of a smoothing state (lgssm.jl:111-113 through lgc.jl:46-52 with the replaced noise): mean = H' m + h, var = H' P H + R'
template <int D> TGP_HD void emit(const double* H, double hh, double Rn, const State<D>& xs, double& mean, double& var) {
    double mu = hh, v = Rn;
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        double acc = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(H[k], xs.P[pidx(k, j)], acc);
        v = ::fma(acc, H[j], v);
        mu = ::fma(H[j], xs.m[j], mu);
    }
    mean = mu;
    var = v;
}

// How far apart two states are, relative to the size of a state: what the checks of a forgotten start compare with mc.tol.
template <int D> TGP_HD double state_distance(const ModelC<D>& mc, const State<D>& a, const State<D>& b) {
    double worst = 0.0;
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        const double sc = ::sqrt(mc.gP[pidx(i, i)]) + ::fabs(a.m[i]) + ::fabs(b.m[i]);
        const double r = ::fabs(a.m[i] - b.m[i]) / sc;
        worst = r > worst ? r : worst;      // (a NaN on either side compares false everywhere: caught by the caller's finite test)
    }
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            const double sc = ::sqrt(mc.gP[pidx(i, i)] * mc.gP[pidx(j, j)]);
            const double r = ::fabs(a.P[pidx(i, j)] - b.P[pidx(i, j)]) / sc;
            worst = r > worst ? r : worst;
        }
    return worst;
}

// ---- the inputs of one step, as every pass sees them ------------------------------------------------------------------------------
struct Streams {
    const double* y = nullptr;
    const uint8_t* mask = nullptr;      // 1 = missing (nullptr: none)
    const double* R = nullptr;          // per step (nullptr: mc.R)
    const double* hh = nullptr;         // per step (nullptr: mc.hh)
    const double* tau = nullptr;        // SDE: gap to the previous time stamp (entry 0 unused: the first transition is explicit)
    const double* Rnew = nullptr;       // per step, or one value (rnew_per_step == 0)
    int rnew_per_step = 0;
};

// ---- the runs of one lane (the kernel of tgp_sweep.hip and tests/hostsim/sweepsim.cpp call the same code) ---------------------------------
template <int D> struct KArgs {
    ModelC<D> mc;
    Streams st;
    long long T;
    int C, W, Wb;               // steps per chunk, forward / backward warm-up: multiples of 8
    long long nchunks;
    double* mean;
    double* var;
    double* ckpt;               // [wave][block][component][lane]
    double* part;               // [wave][4]: share of the log marginal likelihood, status bits, forward / backward distance (pinned host memory)
};

// steps per block: a checkpoint of the forward run every B steps; the block's B filtering states sit in LDS during the backward run
template <int D> struct Geo {
    static constexpr int B = D <= 3 ? 8 : 4;
};

// Register residency of the model's shared blocks inside the runs.  Measured (scripts/ubench/fp64_issue.hip, one wave per SIMD): dependent
// v_fma_f64 issue back to back at 4.6 cycles, but a scalar load whose value is used right away costs ~100 cycles -- and the first version of
// this engine re-read its constants from the argument segment in every step (the compiler prefers re-loading an invariant value to keeping
// it).  A value that went through one of these statements is opaque to the optimiser: it stays in a register of the named file.
#if defined(__HIP_DEVICE_COMPILE__)
#define TGP_PIN_V(x) asm volatile("" : "+v"(x))
#define TGP_PIN_S(x) asm volatile("" : "+s"(x))
#else
#define TGP_PIN_V(x) ((void)0)
#define TGP_PIN_S(x) ((void)0)
#endif

// The model as the runs hold it: multipliers wave-uniform (scalar registers), addends in vector registers (an instruction takes ONE scalar
// operand).  SDE models: `A` is not kept (a step builds its own from tau; the series' first transition is read from the arguments where needed).
template <int D, bool SDE> struct ModelR {
    double A[SDE ? 1 : D * D];
    double a[D];
    double Qg[SD<D>::DS];                 // LTI: Q;  SDE: Pinf
    double H[D];
    double lam[SDE ? D : 1], N1[SDE ? D * D : 1], N2[SDE ? D * D : 1];
    double hh, R;
    TGP_HD void init(const ModelC<D>& mc) {
        if constexpr (!SDE) {
            TGP_UNROLL for (int i = 0; i < D * D; ++i) { A[i] = mc.A[i]; TGP_PIN_S(A[i]); }
            lam[0] = N1[0] = N2[0] = 0.0;
        } else {
            A[0] = 0.0;
            TGP_UNROLL for (int i = 0; i < D; ++i) { lam[i] = mc.lam[i]; TGP_PIN_S(lam[i]); }
            TGP_UNROLL for (int i = 0; i < D * D; ++i) { N1[i] = mc.N1[i]; N2[i] = mc.N2[i]; TGP_PIN_S(N1[i]); TGP_PIN_S(N2[i]); }
        }
        TGP_UNROLL for (int i = 0; i < D; ++i) { a[i] = mc.a[i]; H[i] = mc.H[i]; TGP_PIN_V(a[i]); TGP_PIN_S(H[i]); }
        TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) { Qg[i] = SDE ? mc.gP[i] : mc.Q[i]; TGP_PIN_V(Qg[i]); }
        hh = mc.hh;
        R = mc.R;
        TGP_PIN_V(hh);
        TGP_PIN_V(R);
    }
};

// the transition matrix of step t (tau: the gap in front of it)
template <int D, bool SDE> TGP_HD void step_A(const ModelC<D>& mc, const ModelR<D, SDE>& mr, double tau, bool first, double* A) {
    if constexpr (SDE) {
        double e[D];
        e[0] = ::exp(-mr.lam[0] * tau);
        TGP_UNROLL for (int i = 1; i < D; ++i) e[i] = (mr.lam[i] == mr.lam[i - 1]) ? e[i - 1] : ::exp(-mr.lam[i] * tau);     // (wave-uniform: one exp per block)
        const double t2 = tau * tau;
        TGP_UNROLL for (int j = 0; j < D; ++j)
            TGP_UNROLL for (int i = 0; i < D; ++i) A[i + j * D] = e[i] * ::fma(t2, mr.N2[i + j * D], ::fma(tau, mr.N1[i + j * D], i == j ? 1.0 : 0.0));
        if (first) {      // (the series' first step only: one lane of one wave, once)
            TGP_UNROLL for (int i = 0; i < D * D; ++i) A[i] = mc.A[i];
        }
    } else {
        TGP_UNROLL for (int i = 0; i < D * D; ++i) A[i] = mr.A[i];
    }
}

// predict (lgc.jl:46-52) on the register-resident model.  AP_out (optional, full d x d): A Symmetric(P) of the INCOMING covariance -- what
// invert_dynamics multiplies again (lgssm.jl:234).
template <int D, bool SDE> TGP_HD void predict_r(const ModelR<D, SDE>& mr, const double* A, double* m, double* P, double* AP_out = nullptr) {
    double mp[D];
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = mr.a[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(A[i + k * D], m[k], acc);
        mp[i] = acc;
    }
    TGP_UNROLL for (int i = 0; i < D; ++i) m[i] = mp[i];
    double AX[D * D], Pn[SD<D>::DS];
    if constexpr (SDE) {
        if (AP_out) {      // A P and A Pinf separately: the smoother needs A P itself
            double AG[D * D];
            mul_A_sym<D>(A, P, AP_out);
            mul_A_sym<D>(A, mr.Qg, AG);
            TGP_UNROLL for (int i = 0; i < D * D; ++i) AX[i] = AP_out[i] - AG[i];
        } else {
            double Dm[SD<D>::DS];
            TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) Dm[i] = P[i] - mr.Qg[i];
            mul_A_sym<D>(A, Dm, AX);
        }
    } else {
        mul_A_sym<D>(A, P, AX);
        if (AP_out) { TGP_UNROLL for (int i = 0; i < D * D; ++i) AP_out[i] = AX[i]; }
    }
    mul_AXAt_plus<D>(AX, A, mr.Qg, Pn);
    TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) P[i] = Pn[i];
}

// One step of the reverse-time recursion on the register-resident model (see smooth_step above: the same arithmetic)
template <int D, bool SDE> TGP_HD void smooth_step_r(const ModelR<D, SDE>& mr, const double* A, const State<D>& xf, State<D>& xs, bool& ok) {
    constexpr int DS = SD<D>::DS;
    double mp[D], Pp[DS], AP[D * D];
    TGP_UNROLL for (int i = 0; i < D; ++i) mp[i] = xf.m[i];
    TGP_UNROLL for (int i = 0; i < DS; ++i) Pp[i] = xf.P[i];
    predict_r<D, SDE>(mr, A, mp, Pp, AP);
    double U[D * D], inv[D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < j; ++i) {
            double acc = Pp[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], U[k + j * D], acc);
            U[i + j * D] = acc * inv[i];
        }
        double acc = Pp[pidx(j, j)] + kJitter;
        TGP_UNROLL for (int k = 0; k < j; ++k) acc = ::fma(-U[k + j * D], U[k + j * D], acc);
        ok = ok && (acc > 0.0);
        double s, rs;
        fast_sqrt_rsqrt(acc, s, rs);
        U[j + j * D] = s;
        inv[j] = rs;
    }
    double W[D * D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = AP[i + j * D];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], W[k + j * D], acc);
            W[i + j * D] = acc * inv[i];
        }
        TGP_UNROLL for (int i = D - 1; i >= 0; --i) {
            double acc = W[i + j * D];
            TGP_UNROLL for (int k = i + 1; k < D; ++k) acc = ::fma(-U[i + k * D], W[k + j * D], acc);
            W[i + j * D] = acc * inv[i];
        }
    }
    double dm[D], Dm[DS];
    TGP_UNROLL for (int i = 0; i < D; ++i) dm[i] = xs.m[i] - mp[i];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) Dm[pidx(i, j)] = xs.P[pidx(i, j)] - Pp[pidx(i, j)] - (i == j ? kJitter : 0.0);
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = xf.m[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(W[k + i * D], dm[k], acc);
        xs.m[i] = acc;
    }
    double GD[D * D];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(W[k + i * D], Dm[pidx(k, j)], acc);
            GD[i + j * D] = acc;
        }
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            double acc = xf.P[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(GD[i + k * D], W[k + j * D], acc);
            xs.P[pidx(i, j)] = acc;
        }
}

// The reverse-time recursion over a window of steps [t0, te), composed FORWARDS (round 5, later): xs_(t0) = E xs_(te-1) + g,
// Ps_(t0) = E Ps_(te-1) E' + L.  The forward run has, at step t, everything step t - 1's reverse-time element needs (the filtering state in
// front of the predict, A P, the predicted state: invert_dynamics lgssm.jl:231-238), so the smoothing state a chunk hands to the lane before
// it -- the backward warm-up's result -- comes out of the forward run of the chunk's first Wb steps at ~190 instructions per step, instead
// of a backward pass of its own over them (recompute + reverse step: ~330).
template <int D> struct RevAcc {
    double E[D * D], g[D], L[SD<D>::DS];
    TGP_HD void reset() {
        TGP_UNROLL for (int j = 0; j < D; ++j) TGP_UNROLL for (int i = 0; i < D; ++i) E[i + j * D] = i == j ? 1.0 : 0.0;
        TGP_UNROLL for (int i = 0; i < D; ++i) g[i] = 0.0;
        TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) L[i] = 0.0;
    }
    // xs_(t0) from the window's last filtering state
    TGP_HD void finish(const State<D>& xl, State<D>& out) const {
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = g[i];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(E[i + k * D], xl.m[k], acc);
            out.m[i] = acc;
        }
        double EP[D * D];
        mul_A_sym<D>(E, xl.P, EP);
        mul_AXAt_plus<D>(EP, E, L, out.P);
    }
};
// xf: filtering state of step t - 1; (mp, Pp): predicted state of step t; AP = A Symmetric(xf.P).  Appends step t - 1's element.
template <int D> TGP_HD void rev_append(const State<D>& xf, const double* mp, const double* Pp, const double* AP, RevAcc<D>& ra, bool& ok) {
    constexpr int DS = SD<D>::DS;
    double U[D * D], inv[D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < j; ++i) {
            double acc = Pp[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], U[k + j * D], acc);
            U[i + j * D] = acc * inv[i];
        }
        double acc = Pp[pidx(j, j)] + kJitter;
        TGP_UNROLL for (int k = 0; k < j; ++k) acc = ::fma(-U[k + j * D], U[k + j * D], acc);
        ok = ok && (acc > 0.0);
        double sq, rs;
        fast_sqrt_rsqrt(acc, sq, rs);
        U[j + j * D] = sq;
        inv[j] = rs;
    }
    double W[D * D], Z[D * D];      // Z = U^-T (A Pf) = U G';  W = U^-1 Z = G'
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = AP[i + j * D];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], Z[k + j * D], acc);
            Z[i + j * D] = acc * inv[i];
        }
        TGP_UNROLL for (int i = D - 1; i >= 0; --i) {
            double acc = Z[i + j * D];
            TGP_UNROLL for (int k = i + 1; k < D; ++k) acc = ::fma(-U[i + k * D], W[k + j * D], acc);
            W[i + j * D] = acc * inv[i];
        }
    }
    // g_t = mf - G mp;  L_t = Pf - (U G')'(U G')   (lgssm.jl:236-237)
    double gt[D], Lt[DS];
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = xf.m[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(-W[k + i * D], mp[k], acc);
        gt[i] = acc;
    }
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            double acc = xf.P[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(-Z[k + i * D], Z[k + j * D], acc);
            Lt[pidx(i, j)] = acc;
        }
    // g += E g_t;  L += E L_t E';  E <- E G      (G[i][k] = W[k + i D])
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = ra.g[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(ra.E[i + k * D], gt[k], acc);
        ra.g[i] = acc;
    }
    double EL[D * D], Ln[DS], En[D * D];
    mul_A_sym<D>(ra.E, Lt, EL);
    mul_AXAt_plus<D>(EL, ra.E, ra.L, Ln);
    TGP_UNROLL for (int i = 0; i < DS; ++i) ra.L[i] = Ln[i];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(ra.E[i + k * D], W[j + k * D], acc);      // (E G)[i][j] = sum_k E[i][k] G[k][j], G[k][j] = W[j + k D]
            En[i + j * D] = acc;
        }
    TGP_UNROLL for (int i = 0; i < D * D; ++i) ra.E[i] = En[i];
}

// Inputs of the B steps of a block.  XS bit 0: the noise variance is per step, bit 1: the emission offset is.  A lane's B steps are B
// consecutive values of each stream: the loads of a block are issued together (one cache line per lane and stream: the first load brings
// it, the others hit -- one load per step, spread over the block, was measured 25 % slower: the line is gone from the 32 KB L1 by then),
// a whole block ahead of their use (cur / nxt).
template <int D, bool SDE, int XS, int B> struct Inputs {
    double y[B];
    double R[(XS & 1) ? B : 1];
    double hh[(XS & 2) ? B : 1];
    double tau[SDE ? B : 1];
    unsigned mk[B];      // the steps' mask bytes as loaded (compared where a step uses them: a comparison at the load would wait for it)
    TGP_HD bool obs(int j, long long t, long long T) const { return t < T && mk[j] == 0u; }      // (steps behind the series are missing: the runs pad their last block)
};
TGP_HD long long clamp_t(long long t, long long T) { return t < 0 ? 0 : (t >= T ? T - 1 : t); }

template <int D, bool SDE, int XS, int B> TGP_HD void load_inputs(const KArgs<D>& ka, long long tb, Inputs<D, SDE, XS, B>& in) {
    long long tc[B];
    TGP_UNROLL for (int j = 0; j < B; ++j) tc[j] = clamp_t(tb + j, ka.T);
    TGP_UNROLL for (int j = 0; j < B; ++j) in.y[j] = ka.st.y[tc[j]];
    if constexpr (SDE) { TGP_UNROLL for (int j = 0; j < B; ++j) in.tau[j] = ka.st.tau[tc[j]]; }
    if constexpr ((XS & 1) != 0) { TGP_UNROLL for (int j = 0; j < B; ++j) in.R[j] = ka.st.R[tc[j]]; }
    if constexpr ((XS & 2) != 0) { TGP_UNROLL for (int j = 0; j < B; ++j) in.hh[j] = ka.st.hh[tc[j]]; }
    TGP_UNROLL for (int j = 0; j < B; ++j) in.mk[j] = 0u;
    if (ka.st.mask != nullptr) { TGP_UNROLL for (int j = 0; j < B; ++j) in.mk[j] = ka.st.mask[tc[j]]; }
}

// One forward run of a lane: `nblk` blocks of B steps from step ts on (ts a multiple of 8, possibly negative); the blocks that start in
// [lo, hi) are processed, whole (lo, hi multiples of 8; steps behind the series' end are missing).  x: filtering state in front of step
// max(ts, lo) on entry, behind the last processed step on return.  acc: the log marginal likelihood's sums (want_lml: the logs are taken).
// ckpt (null: none): the state in front of every block is kept, [block][component][lane].
// REV: the reverse-time recursion over the steps (rev_t0, rev_te) is composed on the way (see RevAcc: rev holds the composition so far, the run may
// be one of several over the window); *rev_out = the smoothing state of step rev_t0 it gives from the filtering state of step rev_te - 1.
template <int D, bool SDE, int XS, int B, bool REV = false>
TGP_HD void forward_run(const KArgs<D>& ka, const ModelR<D, SDE>& mr, long long ts, int nblk, long long lo, long long hi, State<D>& x, LmlAcc& acc,
                        bool want_lml, double* ckpt, int lane, bool& ok, RevAcc<D>* rev = nullptr, long long rev_t0 = 0, long long rev_te = 0,
                        State<D>* rev_out = nullptr) {
    constexpr int NS = SD<D>::NS;
    Inputs<D, SDE, XS, B> in, nx;
    load_inputs<D, SDE, XS, B>(ka, ts, in);
    for (int b = 0; b < nblk; ++b) {
        const long long tb = ts + (long long)b * B;
        load_inputs<D, SDE, XS, B>(ka, tb + B, nx);      // in flight while this block computes (behind the last block: clamped, unused)
        TGP_ISSUE_BARRIER();
        if (ckpt != nullptr) {
            double* q = ckpt + (size_t)b * NS * 64 + lane;
            TGP_UNROLL for (int k = 0; k < D; ++k) q[(size_t)k * 64] = x.m[k];
            TGP_UNROLL for (int k = 0; k < SD<D>::DS; ++k) q[(size_t)(D + k) * 64] = x.P[k];
        }
        if (tb >= lo && tb < hi) {
            TGP_UNROLL for (int j = 0; j < B; ++j) {
                double A[D * D];
                step_A<D, SDE>(ka.mc, mr, SDE ? in.tau[j] : 0.0, SDE && tb + j == 0, A);
                if constexpr (REV) {
                    const long long t = tb + j;
                    State<D> xf = x;
                    double AP[D * D];
                    predict_r<D, SDE>(mr, A, x.m, x.P, AP);
                    if (t > rev_t0 && t < rev_te) rev_append<D>(xf, x.m, x.P, AP, *rev, ok);
                    update<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, t, ka.T), x.m, x.P, &acc, ok);
                    if (t == rev_te - 1) rev->finish(x, *rev_out);
                } else {
                    predict_r<D, SDE>(mr, A, x.m, x.P);
                    update<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, tb + j, ka.T), x.m, x.P, &acc, ok);
                }
            }
        }
        if (want_lml) acc.flush();      // (wave-uniform)
        else acc.prod = 1.0;
        in = nx;
    }
}

// One backward run of a lane over the blocks nblk - 1 .. 0 of its chunk (first step t0, a multiple of 8): the steps below hi are smoothed.
// fresh: the run starts at step hi - 1 from that step's filtering state (the end of the series, or a warm-up); otherwise xs holds the smoothing
// state of step hi (the next lane's first step).  On return xs is the smoothing state of step t0.  emit_out: write mean / var of the steps.
// The filtering states of a block are recomputed from its checkpoint into LDS (sF: [step][component][lane]) -- with the steps behind the
// series' end as missing ones, exactly as the forward run took them.
template <int D, bool SDE, int XS, int B>
TGP_HD void backward_run(const KArgs<D>& ka, const ModelR<D, SDE>& mr, long long t0, int nblk, long long hi, bool fresh, State<D>& xs, bool emit_out,
                         const double* ckpt, double* sF, int lane, bool& ok) {
    constexpr int NS = SD<D>::NS, DS = SD<D>::DS;
    const long long T = ka.T;
    Inputs<D, SDE, XS, B> in, nx;
    double tau_next = 0.0;      // gap in front of the step behind the block in hand
    const long long tlast = t0 + (long long)(nblk - 1) * B;
    if (SDE) tau_next = ka.st.tau[clamp_t(tlast + B, T)];
    load_inputs<D, SDE, XS, B>(ka, tlast, in);
    State<D> ck, ckN;
    {
        const double* q = ckpt + (size_t)(nblk - 1) * NS * 64 + lane;
        TGP_UNROLL for (int k = 0; k < D; ++k) ck.m[k] = q[(size_t)k * 64];
        TGP_UNROLL for (int k = 0; k < DS; ++k) ck.P[k] = q[(size_t)(D + k) * 64];
    }
    for (int b = nblk - 1; b >= 0; --b) {
        const long long tb = t0 + (long long)b * B;
        load_inputs<D, SDE, XS, B>(ka, tb - B, nx);      // the next block (block b - 1): in flight through this one
        {
            const double* q = ckpt + (size_t)(b > 0 ? b - 1 : 0) * NS * 64 + lane;
            TGP_UNROLL for (int k = 0; k < D; ++k) ckN.m[k] = q[(size_t)k * 64];
            TGP_UNROLL for (int k = 0; k < DS; ++k) ckN.P[k] = q[(size_t)(D + k) * 64];
        }
        TGP_ISSUE_BARRIER();
        // ---- the block's filtering states, forwards from its checkpoint
        State<D> x = ck;
        TGP_UNROLL for (int j = 0; j < B; ++j) {
            double A[D * D];
            step_A<D, SDE>(ka.mc, mr, SDE ? in.tau[j] : 0.0, SDE && tb + j == 0, A);
            predict_r<D, SDE>(mr, A, x.m, x.P);
            update<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, tb + j, T), x.m, x.P, (LmlAcc*)nullptr, ok);
            TGP_UNROLL for (int k = 0; k < D; ++k) sF[(j * NS + k) * 64 + lane] = x.m[k];
            TGP_UNROLL for (int k = 0; k < DS; ++k) sF[(j * NS + D + k) * 64 + lane] = x.P[k];
        }
        // ---- backwards through the block (the barrier: the states are to be READ BACK from LDS -- without it the optimiser forwards the eight
        // states of the first half to the second through registers, which is the register pressure the LDS buffer is there to remove)
        TGP_ISSUE_BARRIER();
        double om[B], ov[B];
        TGP_UNROLL for (int j = B - 1; j >= 0; --j) {
            const long long t = tb + j;
            om[j] = 0.0;
            ov[j] = 0.0;
            if (t < hi) {
                double rn = 0.0;
                if (emit_out) rn = ka.st.Rnew[ka.st.rnew_per_step ? t : 0];      // (asked for here, used at the end of the step)
                State<D> xf;
                TGP_UNROLL for (int k = 0; k < D; ++k) xf.m[k] = sF[(j * NS + k) * 64 + lane];
                TGP_UNROLL for (int k = 0; k < DS; ++k) xf.P[k] = sF[(j * NS + D + k) * 64 + lane];
                if (fresh && t == hi - 1) {
                    xs = xf;
                } else {
                    double A[D * D];
                    step_A<D, SDE>(ka.mc, mr, SDE ? (j == B - 1 ? tau_next : in.tau[j + 1 < B ? j + 1 : j]) : 0.0, false, A);
                    smooth_step_r<D, SDE>(mr, A, xf, xs, ok);
                }
                if (emit_out) emit<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, rn, xs, om[j], ov[j]);
            }
        }
        if (emit_out) {
#if defined(__HIP_DEVICE_COMPILE__)
            // A lane's B outputs are B consecutive values of each array, 8 C bytes from its neighbour's: stored by their owners they are
            // 64 pieces of 8 bytes per instruction (measured: the main backward pass took 2.4 x the warm-up pass, which stores nothing).
            // Through LDS instead (the block's states have been read: their buffer is free): rows of B values, B lanes store one row's
            // B x 8 consecutive bytes.
            constexpr int LD = B + 1, RPI = 64 / B;      // row stride in doubles (bank spread), rows per store instruction
            const unsigned long long emits = __builtin_amdgcn_ballot_w64(hi > t0);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            TGP_UNROLL for (int j = 0; j < B; ++j) {
                sF[lane * LD + j] = om[j];
                sF[64 * LD + lane * LD + j] = ov[j];
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // first step of lane 0's chunk, from lane 1's (always a chunk of the series; a lane without one has t0 = 0)
            const long long tw0 = (((long long)__builtin_amdgcn_readlane((int)(t0 >> 32), 1) << 32) | (unsigned)__builtin_amdgcn_readlane((int)t0, 1)) - ka.C;
            const bool wide = (((unsigned long long)ka.mean | (unsigned long long)ka.var) & 15ull) == 0ull;      // (wave-uniform)
            if (wide) {      // 16-byte pieces: B / 2 lanes per row, 128 / B rows per instruction
                constexpr int PPR = B / 2, RPW = 64 / PPR;
                const int pc = lane % PPR, rw = lane / PPR;
                TGP_UNROLL for (int k = 0; k < PPR; ++k) {
                    const int r = rw + RPW * k;
                    const long long t = tw0 + (long long)r * ka.C + (tb - t0) + 2 * pc;
                    double2 vm, vv;
                    vm.x = sF[r * LD + 2 * pc];
                    vm.y = sF[r * LD + 2 * pc + 1];
                    vv.x = sF[64 * LD + r * LD + 2 * pc];
                    vv.y = sF[64 * LD + r * LD + 2 * pc + 1];
                    if (((emits >> r) & 1ull) != 0ull) {
                        if (t + 1 < T) {
                            *reinterpret_cast<double2*>(ka.mean + t) = vm;
                            *reinterpret_cast<double2*>(ka.var + t) = vv;
                        } else if (t < T) {
                            ka.mean[t] = vm.x;
                            ka.var[t] = vv.x;
                        }
                    }
                }
            } else {
                const int e = lane % B, r0 = lane / B;
                TGP_UNROLL for (int k = 0; k < B; ++k) {
                    const int r = r0 + RPI * k;
                    const long long t = tw0 + (long long)r * ka.C + (tb - t0) + e;
                    const double vm = sF[r * LD + e], vv = sF[64 * LD + r * LD + e];
                    if (((emits >> r) & 1ull) != 0ull && t < T) {
                        ka.mean[t] = vm;
                        ka.var[t] = vv;
                    }
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
#else
            TGP_UNROLL for (int j = 0; j < B; ++j) {
                if (tb + j < hi) {
                    ka.mean[tb + j] = om[j];
                    ka.var[tb + j] = ov[j];
                }
            }
#endif
        }
        if (SDE) tau_next = in.tau[0];
        in = nx;
        ck = ckN;
    }
}

// ---- posterior draws (k_sweep_draw): rand of the reverse-time model (lgssm.jl:65-91 on :193-238) without writing it ----------------
// Index roles as oracle/lgssm_ref.py posterior / rand: the reverse-time model's start is x_(T-1) ~ N(mf, Pf) of the last step (rand_x0: jitter
// 1e-12); its transition of step t >= 1 takes x_t to x_(t-1) = G_t x_t + g_t + chol(L_t + 1e-9 I).U' eps_t[t] (lgc.jl:84-87), with
// (G_t, g_t, L_t) = invert_dynamics of step t - 1's filtering state and step t's predicted one; step 0's transition is drawn and discarded.
// The emission of step t is H x_t + h_t + sqrt(Rnew_t) eps_e[t] (scalar: lgc.jl:241-243, no jitter).
constexpr double kJitterDraw = 1e-9, kJitterStart = 1e-12;

// upper Cholesky factor of Symmetric(M) + jit I (M packed): U[k + j D], k <= j, and the reciprocal pivots
template <int D> TGP_HD void chol_upper(const double* M, double jit, double* U, double* inv, bool& ok) {
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < j; ++i) {
            double acc = M[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], U[k + j * D], acc);
            U[i + j * D] = acc * inv[i];
        }
        double acc = M[pidx(j, j)] + jit;
        TGP_UNROLL for (int k = 0; k < j; ++k) acc = ::fma(-U[k + j * D], U[k + j * D], acc);
        ok = ok && (acc > 0.0);
        double s, rs;
        fast_sqrt_rsqrt(acc, s, rs);
        U[j + j * D] = s;
        inv[j] = rs;
    }
}
// out = U' e
template <int D> TGP_HD void mul_Ut(const double* U, const double* e, double* out) {
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = 0.0;
        TGP_UNROLL for (int k = 0; k <= i; ++k) acc = ::fma(U[k + i * D], e[k], acc);
        out[i] = acc;
    }
}

// x_(T-1) = mf + chol(Pf + 1e-12 I).U' eps_0
template <int D> TGP_HD void draw_start(const State<D>& xf, const double* eps0, double* x, bool& ok) {
    double U[D * D], inv[D], nz[D];
    chol_upper<D>(xf.P, kJitterStart, U, inv, ok);
    mul_Ut<D>(U, eps0, nz);
    TGP_UNROLL for (int i = 0; i < D; ++i) x[i] = xf.m[i] + nz[i];
}

// The reverse-time element of step t - 1: xf its filtering state, (mp, Pp) step t's predicted state, AP = A Symmetric(xf.P), eps = eps_t[t].
// Wt = G' (G[i][k] = Wt[k + i D]); nz = chol(L + 1e-9 I).U' eps, L = Pf - (U G')'(U G').
template <int D> TGP_HD void draw_elem(const State<D>& xf, const double* Pp, const double* AP, const double* eps, double* Wt, double* nz, bool& ok) {
    constexpr int DS = SD<D>::DS;
    double U[D * D], inv[D];
    chol_upper<D>(Pp, kJitter, U, inv, ok);
    double Z[D * D];      // Z = U^-T (A Pf) = U G';  Wt = U^-1 Z
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = AP[i + j * D];
            TGP_UNROLL for (int k = 0; k < i; ++k) acc = ::fma(-U[k + i * D], Z[k + j * D], acc);
            Z[i + j * D] = acc * inv[i];
        }
        TGP_UNROLL for (int i = D - 1; i >= 0; --i) {
            double acc = Z[i + j * D];
            TGP_UNROLL for (int k = i + 1; k < D; ++k) acc = ::fma(-U[i + k * D], Wt[k + j * D], acc);
            Wt[i + j * D] = acc * inv[i];
        }
    }
    double Lt[DS];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            double acc = xf.P[pidx(i, j)];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(-Z[k + i * D], Z[k + j * D], acc);
            Lt[pidx(i, j)] = acc;
        }
    double UL[D * D], invL[D];
    chol_upper<D>(Lt, kJitterDraw, UL, invL, ok);
    mul_Ut<D>(UL, eps, nz);
}

// One step of the walk on the register-resident model: xf = filtering state of step t, A = transition of step t + 1, eps = eps_t[t + 1];
// x = x_(t+1) on entry, x_t on return:  x_t = mf + G (x_(t+1) - mp) + chol(L + 1e-9 I).U' eps
template <int D, bool SDE> TGP_HD void draw_step_r(const ModelR<D, SDE>& mr, const double* A, const State<D>& xf, double* x, const double* eps, bool& ok) {
    constexpr int DS = SD<D>::DS;
    double mp[D], Pp[DS], AP[D * D];
    TGP_UNROLL for (int i = 0; i < D; ++i) mp[i] = xf.m[i];
    TGP_UNROLL for (int i = 0; i < DS; ++i) Pp[i] = xf.P[i];
    predict_r<D, SDE>(mr, A, mp, Pp);      // (the filter's own predict, to the bit: see forward_run_draw)
    mul_A_sym<D>(A, xf.P, AP);
    double Wt[D * D], nz[D], dm[D];
    draw_elem<D>(xf, Pp, AP, eps, Wt, nz, ok);
    TGP_UNROLL for (int i = 0; i < D; ++i) dm[i] = x[i] - mp[i];
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double acc = xf.m[i] + nz[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(Wt[k + i * D], dm[k], acc);
        x[i] = acc;
    }
}

// The walk over a window of steps [t0, te), composed FORWARDS as RevAcc composes the smoother's: x_(t0) = E x_(te-1) + g, with g carrying the
// noise terms (no covariance: the walk is a sample path).
template <int D> struct DrawAcc {
    double E[D * D], g[D];
    TGP_HD void reset() {
        TGP_UNROLL for (int j = 0; j < D; ++j) TGP_UNROLL for (int i = 0; i < D; ++i) E[i + j * D] = i == j ? 1.0 : 0.0;
        TGP_UNROLL for (int i = 0; i < D; ++i) g[i] = 0.0;
    }
    // appends step t - 1's element (arguments as draw_elem; mp: step t's predicted mean)
    TGP_HD void append(const State<D>& xf, const double* mp, const double* Pp, const double* AP, const double* eps, bool& ok) {
        double Wt[D * D], nz[D], gt[D], En[D * D];
        draw_elem<D>(xf, Pp, AP, eps, Wt, nz, ok);
        TGP_UNROLL for (int i = 0; i < D; ++i) {      // g_t = mf - G mp + noise
            double acc = xf.m[i] + nz[i];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(-Wt[k + i * D], mp[k], acc);
            gt[i] = acc;
        }
        TGP_UNROLL for (int i = 0; i < D; ++i) {      // g += E g_t;  E <- E G
            double acc = g[i];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(E[i + k * D], gt[k], acc);
            g[i] = acc;
        }
        TGP_UNROLL for (int j = 0; j < D; ++j)
            TGP_UNROLL for (int i = 0; i < D; ++i) {
                double acc = 0.0;
                TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(E[i + k * D], Wt[j + k * D], acc);
                En[i + j * D] = acc;
            }
        TGP_UNROLL for (int i = 0; i < D * D; ++i) E[i] = En[i];
    }
    // x_(t0) from the window's last step: its filtering mean (zero deviation), or the true x_(T-1) where the window reaches the series' end
    TGP_HD void finish(const State<D>& xl, bool at_end, const double* eps0, double* out, bool& ok) const {
        double xe[D], xd[D];
        bool okd = true;
        draw_start<D>(xl, eps0, xd, okd);
        if (at_end) ok = ok && okd;
        TGP_UNROLL for (int i = 0; i < D; ++i) xe[i] = at_end ? xd[i] : xl.m[i];
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double acc = g[i];
            TGP_UNROLL for (int k = 0; k < D; ++k) acc = ::fma(E[i + k * D], xe[k], acc);
            out[i] = acc;
        }
    }
};

// distance of two sample states, on the scale of state_distance's mean part
template <int D> TGP_HD double draw_distance(const ModelC<D>& mc, const double* a, const double* b) {
    double worst = 0.0;
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        const double sc = ::sqrt(mc.gP[pidx(i, i)]) + ::fabs(a[i]) + ::fabs(b[i]);
        const double r = ::fabs(a[i] - b[i]) / sc;
        worst = r > worst ? r : worst;
    }
    return worst;
}

// The draw's streams (beside Streams): eps_t [T][D] (row t: the transition out of step t), eps_e [T], eps_0 (the start), the sample path's emissions.
struct DrawArgs {
    const double* eps_t = nullptr;
    const double* eps_e = nullptr;
    double eps_0[4] = {0.0, 0.0, 0.0, 0.0};
    double* y_out = nullptr;
};

// The forward run over a chunk's first blocks with the walk over the steps (rev_t0, rev_te) composed on the way: forward_run<REV> with DrawAcc
// in RevAcc's place.  The filter's steps are the plain ones (predict_r without its A P output, which takes another form for SDE models): the walk over
// the chunk recomputes them from the checkpoints to the bit, so both sides of the draw's hand-over check see the same (G, L) -- L = Pf - (U G')'(U G')
// is a difference of near-equal terms behind a tie (dt = 0), and its rounding under the 1e-9 jitter would otherwise sit in the check.
// *out: x_(rev_t0) from the window's last step (DrawAcc::finish).
template <int D, bool SDE, int XS, int B>
TGP_HD void forward_run_draw(const KArgs<D>& ka, const DrawArgs& da, const ModelR<D, SDE>& mr, long long ts, int nblk, long long lo, long long hi, State<D>& x,
                             double* ckpt, int lane, bool& ok, DrawAcc<D>& dr, long long rev_t0, long long rev_te, double* out) {
    constexpr int NS = SD<D>::NS;
    Inputs<D, SDE, XS, B> in, nx;
    load_inputs<D, SDE, XS, B>(ka, ts, in);
    for (int b = 0; b < nblk; ++b) {
        const long long tb = ts + (long long)b * B;
        load_inputs<D, SDE, XS, B>(ka, tb + B, nx);
        double et[D], etn[D];      // the row of eps_t of the step in hand, and the next step's (asked for a step ahead: d doubles in flight, not B d)
        TGP_UNROLL for (int k = 0; k < D; ++k) etn[k] = da.eps_t[(size_t)clamp_t(tb, ka.T) * D + k];
        TGP_ISSUE_BARRIER();
        if (ckpt != nullptr) {
            double* q = ckpt + (size_t)b * NS * 64 + lane;
            TGP_UNROLL for (int k = 0; k < D; ++k) q[(size_t)k * 64] = x.m[k];
            TGP_UNROLL for (int k = 0; k < SD<D>::DS; ++k) q[(size_t)(D + k) * 64] = x.P[k];
        }
        if (tb >= lo && tb < hi) {
            TGP_UNROLL for (int j = 0; j < B; ++j) {
                TGP_UNROLL for (int k = 0; k < D; ++k) et[k] = etn[k];
                if (j + 1 < B) { TGP_UNROLL for (int k = 0; k < D; ++k) etn[k] = da.eps_t[(size_t)clamp_t(tb + j + 1, ka.T) * D + k]; }
                double A[D * D];
                step_A<D, SDE>(ka.mc, mr, SDE ? in.tau[j] : 0.0, SDE && tb + j == 0, A);
                const long long t = tb + j;
                State<D> xf = x;
                predict_r<D, SDE>(mr, A, x.m, x.P);
                if (t > rev_t0 && t < rev_te) {
                    double AP[D * D];
                    mul_A_sym<D>(A, xf.P, AP);
                    dr.append(xf, x.m, x.P, AP, et, ok);
                }
                update<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, t, ka.T), x.m, x.P, (LmlAcc*)nullptr, ok);
                if (t == rev_te - 1) dr.finish(x, rev_te == ka.T, da.eps_0, out, ok);
            }
        }
        in = nx;
    }
}

// The walk of a lane over the blocks nblk - 1 .. 0 of its chunk (backward_run with a sample state in the smoothing state's place): the steps
// below hi are drawn.  fresh: the walk starts at step hi - 1 = T - 1 with draw_start; otherwise x holds x_(hi), the next lane's first step.  On
// return x is x_(t0).
template <int D, bool SDE, int XS, int B>
TGP_HD void backward_run_draw(const KArgs<D>& ka, const DrawArgs& da, const ModelR<D, SDE>& mr, long long t0, int nblk, long long hi, bool fresh, double* x,
                              const double* ckpt, double* sF, int lane, bool& ok) {
    constexpr int NS = SD<D>::NS, DS = SD<D>::DS;
    const long long T = ka.T;
    Inputs<D, SDE, XS, B> in, nx;
    double tau_next = 0.0;      // gap in front of the step behind the block in hand
    const long long tlast = t0 + (long long)(nblk - 1) * B;
    if (SDE) tau_next = ka.st.tau[clamp_t(tlast + B, T)];
    load_inputs<D, SDE, XS, B>(ka, tlast, in);
    State<D> ck, ckN;
    {
        const double* q = ckpt + (size_t)(nblk - 1) * NS * 64 + lane;
        TGP_UNROLL for (int k = 0; k < D; ++k) ck.m[k] = q[(size_t)k * 64];
        TGP_UNROLL for (int k = 0; k < DS; ++k) ck.P[k] = q[(size_t)(D + k) * 64];
    }
    for (int b = nblk - 1; b >= 0; --b) {
        const long long tb = t0 + (long long)b * B;
        load_inputs<D, SDE, XS, B>(ka, tb - B, nx);      // the next block (block b - 1): in flight through this one
        {
            const double* q = ckpt + (size_t)(b > 0 ? b - 1 : 0) * NS * 64 + lane;
            TGP_UNROLL for (int k = 0; k < D; ++k) ckN.m[k] = q[(size_t)k * 64];
            TGP_UNROLL for (int k = 0; k < DS; ++k) ckN.P[k] = q[(size_t)(D + k) * 64];
        }
        // the draws of a step are asked for a step ahead (the block's last step: here, in front of the recomputation): d + 2 doubles in flight
        double et[D], etn[D], ee, een, rn, rnn;
        TGP_UNROLL for (int k = 0; k < D; ++k) etn[k] = da.eps_t[(size_t)clamp_t(tb + B, T) * D + k];
        een = da.eps_e[clamp_t(tb + B - 1, T)];
        rnn = ka.st.Rnew[ka.st.rnew_per_step ? clamp_t(tb + B - 1, T) : 0];
        TGP_ISSUE_BARRIER();
        // ---- the block's filtering states, forwards from its checkpoint
        State<D> xr = ck;
        TGP_UNROLL for (int j = 0; j < B; ++j) {
            double A[D * D];
            step_A<D, SDE>(ka.mc, mr, SDE ? in.tau[j] : 0.0, SDE && tb + j == 0, A);
            predict_r<D, SDE>(mr, A, xr.m, xr.P);
            update<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, tb + j, T), xr.m, xr.P, (LmlAcc*)nullptr, ok);
            TGP_UNROLL for (int k = 0; k < D; ++k) sF[(j * NS + k) * 64 + lane] = xr.m[k];
            TGP_UNROLL for (int k = 0; k < DS; ++k) sF[(j * NS + D + k) * 64 + lane] = xr.P[k];
        }
        TGP_ISSUE_BARRIER();      // (the states are to be read back from LDS: backward_run)
        double oy[B];
        TGP_UNROLL for (int j = B - 1; j >= 0; --j) {
            const long long t = tb + j;
            oy[j] = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) et[k] = etn[k];
            ee = een;
            rn = rnn;
            if (j > 0) {
                TGP_UNROLL for (int k = 0; k < D; ++k) etn[k] = da.eps_t[(size_t)clamp_t(t, T) * D + k];
                een = da.eps_e[clamp_t(t - 1, T)];
                rnn = ka.st.Rnew[ka.st.rnew_per_step ? clamp_t(t - 1, T) : 0];
            }
            if (t < hi) {
                State<D> xf;
                TGP_UNROLL for (int k = 0; k < D; ++k) xf.m[k] = sF[(j * NS + k) * 64 + lane];
                TGP_UNROLL for (int k = 0; k < DS; ++k) xf.P[k] = sF[(j * NS + D + k) * 64 + lane];
                if (fresh && t == hi - 1) {
                    draw_start<D>(xf, da.eps_0, x, ok);
                } else {
                    double A[D * D];
                    step_A<D, SDE>(ka.mc, mr, SDE ? (j == B - 1 ? tau_next : in.tau[j + 1 < B ? j + 1 : j]) : 0.0, false, A);
                    draw_step_r<D, SDE>(mr, A, xf, x, et, ok);
                }
                double mu = (XS & 2) ? in.hh[j] : mr.hh;
                TGP_UNROLL for (int k = 0; k < D; ++k) mu = ::fma(mr.H[k], x[k], mu);
                oy[j] = ::fma(::sqrt(rn), ee, mu);
            }
        }
#if defined(__HIP_DEVICE_COMPILE__)
        {
            // the block's outputs leave through LDS rows of B values (backward_run's tile path, one array)
            constexpr int LD = B + 1, RPI = 64 / B;
            const unsigned long long emits = __builtin_amdgcn_ballot_w64(hi > t0);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            TGP_UNROLL for (int j = 0; j < B; ++j) sF[lane * LD + j] = oy[j];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // first step of lane 0's chunk, from lane 1's (always a chunk of the series; a lane without one has t0 = 0)
            const long long tw0 = (((long long)__builtin_amdgcn_readlane((int)(t0 >> 32), 1) << 32) | (unsigned)__builtin_amdgcn_readlane((int)t0, 1)) - ka.C;
            const bool wide = ((unsigned long long)da.y_out & 15ull) == 0ull;      // (wave-uniform)
            if (wide) {      // 16-byte pieces: B / 2 lanes per row, 128 / B rows per instruction
                constexpr int PPR = B / 2, RPW = 64 / PPR;
                const int pc = lane % PPR, rw = lane / PPR;
                TGP_UNROLL for (int k = 0; k < PPR; ++k) {
                    const int r = rw + RPW * k;
                    const long long t = tw0 + (long long)r * ka.C + (tb - t0) + 2 * pc;
                    double2 vy;
                    vy.x = sF[r * LD + 2 * pc];
                    vy.y = sF[r * LD + 2 * pc + 1];
                    if (((emits >> r) & 1ull) != 0ull) {
                        if (t + 1 < T) *reinterpret_cast<double2*>(da.y_out + t) = vy;
                        else if (t < T) da.y_out[t] = vy.x;
                    }
                }
            } else {
                const int e = lane % B, r0 = lane / B;
                TGP_UNROLL for (int k = 0; k < B; ++k) {
                    const int r = r0 + RPI * k;
                    const long long t = tw0 + (long long)r * ka.C + (tb - t0) + e;
                    const double vy = sF[r * LD + e];
                    if (((emits >> r) & 1ull) != 0ull && t < T) da.y_out[t] = vy;
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
#else
        TGP_UNROLL for (int j = 0; j < B; ++j) {
            if (tb + j < hi) da.y_out[tb + j] = oy[j];
        }
#endif
        if (SDE) tau_next = in.tau[0];
        in = nx;
        ck = ckN;
    }
}

// ---- the adjoint of the filter (k_sweep_adjoint): d logpdf / d (shared blocks, h_t, R_t) in one backward walk -------------------------
// Reverse mode through predict / update above (LTI form).  The walk carries (l, L) = d logpdf / d (m_f, P_f) of the filtering state BEHIND the step in hand
// -- L symmetric, packed: every entry of a covariance counts as a variable of its own and the derivative is kept symmetric, which is what makes the Q and
// x0P gradients come out symmetrised (lgssm.logpdf_adjoint's convention) -- and is zero behind the series' last step.
template <int D> struct Adj {
    double l[D];
    double L[SD<D>::DS];
    TGP_HD void zero() {
        TGP_UNROLL for (int i = 0; i < D; ++i) l[i] = 0.0;
        TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) L[i] = 0.0;
    }
};
// a lane's sums over the steps of its chunk: gA full (column-major), gQ packed, the sums of the per-step gh_t and gR_t
template <int D> struct AdjAcc {
    static constexpr int N = D * D + D + SD<D>::DS + D + 2;
    double gA[D * D], ga[D], gQ[SD<D>::DS], gH[D], gh, gR;
    TGP_HD void zero() {
        TGP_UNROLL for (int i = 0; i < D * D; ++i) gA[i] = 0.0;
        TGP_UNROLL for (int i = 0; i < D; ++i) ga[i] = gH[i] = 0.0;
        TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) gQ[i] = 0.0;
        gh = gR = 0.0;
    }
};

// One step backwards.  xf: the filtering state in FRONT of step t; ad: the adjoint behind it on entry, in front of it on return.  A missing step
// (obs == false; the padded steps behind the series' end are such) passes the adjoint through the predict alone: gh_t = gR_t = 0.
template <int D, bool ACC>
TGP_HD void adjoint_step(const ModelR<D, false>& mr, const State<D>& xf, double hh, double R, double y, bool obs, Adj<D>& ad, AdjAcc<D>* acc, double& gh_t,
                         double& gR_t) {
    constexpr int DS = SD<D>::DS;
    double mp[D], Pp[DS], AP[D * D];
    TGP_UNROLL for (int i = 0; i < D; ++i) mp[i] = xf.m[i];
    TGP_UNROLL for (int i = 0; i < DS; ++i) Pp[i] = xf.P[i];
    predict_r<D, false>(mr, mr.A, mp, Pp, AP);      // (the filter's own predict, to the bit)
    double V[D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        double a = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(mr.H[k], Pp[pidx(k, j)], a);
        V[j] = a;
    }
    double s2 = R, hm = hh;
    TGP_UNROLL for (int k = 0; k < D; ++k) {
        s2 = ::fma(V[k], mr.H[k], s2);
        hm = ::fma(mr.H[k], mp[k], hm);
    }
    const double S = obs ? s2 : 1.0;
    const double iS = obs ? fast_rcp(S) : 0.0;      // (a missing step: every term of the update's adjoint below is a multiple of iS or v)
    const double v = obs ? (y - hm) : 0.0;
    const double viS = v * iS;
    double LV[D], lV = 0.0, VLV = 0.0;
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double a = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(ad.L[pidx(i, k)], V[k], a);
        LV[i] = a;
        lV = ::fma(ad.l[i], V[i], lV);
    }
    TGP_UNROLL for (int i = 0; i < D; ++i) VLV = ::fma(V[i], LV[i], VLV);
    const double vbar = (lV - v) * iS;
    const double Sbar = ::fma(::fma(-lV, v, VLV) * iS, iS, -0.5 * ::fma(-viS, viS, iS));
    double Vb[D];
    TGP_UNROLL for (int i = 0; i < D; ++i) Vb[i] = ::fma(Sbar, mr.H[i], ::fma(ad.l[i], viS, -2.0 * iS * LV[i]));
    gh_t = -vbar;
    gR_t = Sbar;
    double mb[D], Pb[DS];
    TGP_UNROLL for (int i = 0; i < D; ++i) mb[i] = ::fma(-vbar, mr.H[i], ad.l[i]);
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) Pb[pidx(i, j)] = ::fma(0.5, ::fma(Vb[i], mr.H[j], mr.H[i] * Vb[j]), ad.L[pidx(i, j)]);
    if constexpr (ACC) {
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double a = ::fma(Sbar, V[i], -vbar * mp[i]);
            TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(Pp[pidx(i, k)], Vb[k], a);
            acc->gH[i] += a;
            acc->ga[i] += mb[i];
        }
        acc->gh -= vbar;
        acc->gR += Sbar;
        TGP_UNROLL for (int i = 0; i < DS; ++i) acc->gQ[i] += Pb[i];
        TGP_UNROLL for (int k = 0; k < D; ++k)      // gA += mb m' + 2 Pb (A P)
            TGP_UNROLL for (int i = 0; i < D; ++i) {
                double a = 0.0;
                TGP_UNROLL for (int j = 0; j < D; ++j) a = ::fma(Pb[pidx(i, j)], AP[j + k * D], a);
                acc->gA[i + k * D] += ::fma(2.0, a, mb[i] * xf.m[k]);
            }
    }
    // l <- A' mb;  L <- A' Pb A
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double a = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(mr.A[k + i * D], mb[k], a);
        ad.l[i] = a;
    }
    double AtP[D * D];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double a = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(mr.A[k + i * D], Pb[pidx(k, j)], a);
            AtP[i + j * D] = a;
        }
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            double a = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(AtP[i + k * D], mr.A[k + j * D], a);
            ad.L[pidx(i, j)] = a;
        }
}

// How far apart two adjoints are: the dual of state_distance's scaling (l_i sqrt(P_ii), L_ij sqrt(P_ii P_jj), P the stationary prior), absolute -- the
// adjoint of a step is O(1) in these units whatever the model's scale.  Compared with mc.tol_b.
template <int D> TGP_HD double adjoint_distance(const ModelC<D>& mc, const Adj<D>& a, const Adj<D>& b) {
    double sd[D], worst = 0.0;
    TGP_UNROLL for (int i = 0; i < D; ++i) sd[i] = ::sqrt(mc.gP[pidx(i, i)]);
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        const double r = ::fabs(a.l[i] - b.l[i]) * sd[i];
        worst = r > worst ? r : worst;      // (a NaN on either side compares false everywhere: caught by the caller's finite test)
    }
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            const double r = ::fabs(a.L[pidx(i, j)] - b.L[pidx(i, j)]) * (sd[i] * sd[j]);
            worst = r > worst ? r : worst;
        }
    return worst;
}

// The adjoint walk of a lane over the blocks nblk - 1 .. 0 of its chunk (first step t0, a multiple of 8): the steps below hi are walked, from `ad` = the
// adjoint behind step hi - 1; on return `ad` is the adjoint in front of step t0.  The filtering states of a block are recomputed from its checkpoint into
// LDS as backward_run does (sF: [step][component][lane]); step j reads the state in front of it: step j - 1's, the checkpoint for j = 0.
// ACC: the block gradients are summed into *acc, and gh_t / gR_t of every walked step are written where gh_steps / gR_steps are given (a lane's own steps:
// plain stores).
template <int D, int XS, int B, bool ACC>
TGP_HD void adjoint_run(const KArgs<D>& ka, const ModelR<D, false>& mr, long long t0, int nblk, long long hi, Adj<D>& ad, AdjAcc<D>* acc, double* gh_steps,
                        double* gR_steps, const double* ckpt, double* sF, int lane, bool& ok) {
    constexpr int NS = SD<D>::NS, DS = SD<D>::DS;
    const long long T = ka.T;
    Inputs<D, false, XS, B> in, nx;
    const long long tlast = t0 + (long long)(nblk - 1) * B;
    load_inputs<D, false, XS, B>(ka, tlast, in);
    State<D> ck, ckN;
    {
        const double* q = ckpt + (size_t)(nblk > 0 ? nblk - 1 : 0) * NS * 64 + lane;
        TGP_UNROLL for (int k = 0; k < D; ++k) ck.m[k] = q[(size_t)k * 64];
        TGP_UNROLL for (int k = 0; k < DS; ++k) ck.P[k] = q[(size_t)(D + k) * 64];
    }
    for (int b = nblk - 1; b >= 0; --b) {
        const long long tb = t0 + (long long)b * B;
        load_inputs<D, false, XS, B>(ka, tb - B, nx);      // the next block (block b - 1): in flight through this one
        {
            const double* q = ckpt + (size_t)(b > 0 ? b - 1 : 0) * NS * 64 + lane;
            TGP_UNROLL for (int k = 0; k < D; ++k) ckN.m[k] = q[(size_t)k * 64];
            TGP_UNROLL for (int k = 0; k < DS; ++k) ckN.P[k] = q[(size_t)(D + k) * 64];
        }
        TGP_ISSUE_BARRIER();
        // ---- the block's filtering states, forwards from its checkpoint (the last step's is not needed: nothing walks from it)
        State<D> x = ck;
        TGP_UNROLL for (int j = 0; j + 1 < B; ++j) {
            predict_r<D, false>(mr, mr.A, x.m, x.P);
            update<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, tb + j, T), x.m, x.P, (LmlAcc*)nullptr, ok);
            TGP_UNROLL for (int k = 0; k < D; ++k) sF[(j * NS + k) * 64 + lane] = x.m[k];
            TGP_UNROLL for (int k = 0; k < DS; ++k) sF[(j * NS + D + k) * 64 + lane] = x.P[k];
        }
        TGP_ISSUE_BARRIER();      // (the states are to be read back from LDS: backward_run)
        TGP_UNROLL for (int j = B - 1; j >= 0; --j) {
            const long long t = tb + j;
            if (t < hi) {
                State<D> xf = ck;
                if (j > 0) {
                    TGP_UNROLL for (int k = 0; k < D; ++k) xf.m[k] = sF[((j - 1) * NS + k) * 64 + lane];
                    TGP_UNROLL for (int k = 0; k < DS; ++k) xf.P[k] = sF[((j - 1) * NS + D + k) * 64 + lane];
                }
                double gh_t, gR_t;
                adjoint_step<D, ACC>(mr, xf, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, t, T), ad, acc, gh_t, gR_t);
                if constexpr (ACC) {
                    if (gh_steps != nullptr) gh_steps[t] = gh_t;
                    if (gR_steps != nullptr) gR_steps[t] = gR_t;
                }
            }
        }
        in = nx;
        ck = ckN;
    }
}

// ---- the same adjoint for SDE-described models (k_sweep_adjoint_sde): irregular spacing ---------------------------------------------------
// The transition of step t >= 1 is A_t = E (I + tau N1 + tau^2 N2), E = diag(e^(-lam_i tau)), its covariance half runs through Pinf (predict_r<D, true>:
// P_p = A (P - Pinf) A' + Pinf); step 0's is the explicit A1.  G_t = d logpdf / d A_t = mb m' + 2 Pb (A (P - Pinf)) is never stored: it is contracted on the
// spot into the sums over (lam, N1, N2) -- gl_i -= tau sum_j G_ij A_ij, gN1_ij += tau e_i G_ij, gN2_ij += tau^2 e_i G_ij (a tie, tau = 0, adds nothing) --
// and Pinf collects Pb - A' Pb A.  Step 0 gives gA1 = G_0 (one lane of one wave, once: written through a pointer, not summed).
// LDS: the lane's gl and gN2 sums live in shared memory ([component][lane] behind sG) instead of registers (d = 4: the register budget).
TGP_HD constexpr int sde_adjoint_block(int d) { return d <= 2 ? 8 : (d == 3 ? 4 : 2); }
template <int D> struct SdeSums {
    static constexpr bool LDS = D >= 4;
    static constexpr int NL = D + D * D;      // doubles per lane behind sG: gl, gN2
    // steps per block of this pass (Geo<D>::B for the others): shorter blocks at d >= 3 -- half the inputs in flight, half the states in LDS -- are what
    // keeps the kernel under 512 registers without spills; the forward run writes its checkpoints at this pass's own spacing
    static constexpr int B = sde_adjoint_block(D);
};
template <int D> struct AdjAccSde {
    static constexpr int N = D + 2 * D * D + SD<D>::DS + 2 * D + 2;
    double gl[D], gN1[D * D], gN2[D * D], gPinf[SD<D>::DS], ga[D], gH[D], gh, gR;
    TGP_HD void zero() {
        TGP_UNROLL for (int i = 0; i < D * D; ++i) gN1[i] = gN2[i] = 0.0;
        TGP_UNROLL for (int i = 0; i < D; ++i) gl[i] = ga[i] = gH[i] = 0.0;
        TGP_UNROLL for (int i = 0; i < SD<D>::DS; ++i) gPinf[i] = 0.0;
        gh = gR = 0.0;
    }
};

// A_t as step_A<D, true> builds it (the same operations: the same bits), with the exponentials kept
template <int D> TGP_HD void step_A_sde(const ModelC<D>& mc, const ModelR<D, true>& mr, double tau, bool first, double* A, double* e) {
    e[0] = ::exp(-mr.lam[0] * tau);
    TGP_UNROLL for (int i = 1; i < D; ++i) e[i] = (mr.lam[i] == mr.lam[i - 1]) ? e[i - 1] : ::exp(-mr.lam[i] * tau);
    const double t2 = tau * tau;
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) A[i + j * D] = e[i] * ::fma(t2, mr.N2[i + j * D], ::fma(tau, mr.N1[i + j * D], i == j ? 1.0 : 0.0));
    if (first) {
        TGP_UNROLL for (int i = 0; i < D * D; ++i) A[i] = mc.A[i];
    }
}

// One step backwards (adjoint_step's roles).  tau: the gap in front of step t; first: t == 0.  gA1 (ACC): where step 0 writes G_0, D * D doubles.
// sG (ACC, SdeSums<D>::LDS): this lane's slot of the shared sums, component k at sG[k * 64].
template <int D, bool ACC>
TGP_HD void adjoint_step_sde(const ModelC<D>& mc, const ModelR<D, true>& mr, const State<D>& xf, double tau, bool first, double hh, double R, double y, bool obs,
                             Adj<D>& ad, AdjAccSde<D>* acc, double* sG, double* gA1, double& gh_t, double& gR_t) {
    constexpr int DS = SD<D>::DS;
    double A[D * D], e[D];
    step_A_sde<D>(mc, mr, tau, first, A, e);
    // the filter's own predict, to the bit (predict_r<D, true> without AP_out), with A (P - Pinf) kept
    double mp[D], Pp[DS], AX[D * D];
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double a = mr.a[i];
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(A[i + k * D], xf.m[k], a);
        mp[i] = a;
    }
    {
        double Dm[DS];
        TGP_UNROLL for (int i = 0; i < DS; ++i) Dm[i] = xf.P[i] - mr.Qg[i];
        mul_A_sym<D>(A, Dm, AX);
        mul_AXAt_plus<D>(AX, A, mr.Qg, Pp);
    }
    double V[D];
    TGP_UNROLL for (int j = 0; j < D; ++j) {
        double a = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(mr.H[k], Pp[pidx(k, j)], a);
        V[j] = a;
    }
    double s2 = R, hm = hh;
    TGP_UNROLL for (int k = 0; k < D; ++k) {
        s2 = ::fma(V[k], mr.H[k], s2);
        hm = ::fma(mr.H[k], mp[k], hm);
    }
    const double S = obs ? s2 : 1.0;
    const double iS = obs ? fast_rcp(S) : 0.0;
    const double v = obs ? (y - hm) : 0.0;
    const double viS = v * iS;
    double LV[D], lV = 0.0, VLV = 0.0;
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double a = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(ad.L[pidx(i, k)], V[k], a);
        LV[i] = a;
        lV = ::fma(ad.l[i], V[i], lV);
    }
    TGP_UNROLL for (int i = 0; i < D; ++i) VLV = ::fma(V[i], LV[i], VLV);
    const double vbar = (lV - v) * iS;
    const double Sbar = ::fma(::fma(-lV, v, VLV) * iS, iS, -0.5 * ::fma(-viS, viS, iS));
    double Vb[D];
    TGP_UNROLL for (int i = 0; i < D; ++i) Vb[i] = ::fma(Sbar, mr.H[i], ::fma(ad.l[i], viS, -2.0 * iS * LV[i]));
    gh_t = -vbar;
    gR_t = Sbar;
    double mb[D], Pb[DS];
    TGP_UNROLL for (int i = 0; i < D; ++i) mb[i] = ::fma(-vbar, mr.H[i], ad.l[i]);
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) Pb[pidx(i, j)] = ::fma(0.5, ::fma(Vb[i], mr.H[j], mr.H[i] * Vb[j]), ad.L[pidx(i, j)]);
    // l <- A' mb;  L <- A' Pb A
    TGP_UNROLL for (int i = 0; i < D; ++i) {
        double a = 0.0;
        TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(A[k + i * D], mb[k], a);
        ad.l[i] = a;
    }
    double AtP[D * D];
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double a = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(A[k + i * D], Pb[pidx(k, j)], a);
            AtP[i + j * D] = a;
        }
    TGP_UNROLL for (int j = 0; j < D; ++j)
        TGP_UNROLL for (int i = 0; i <= j; ++i) {
            double a = 0.0;
            TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(AtP[i + k * D], A[k + j * D], a);
            ad.L[pidx(i, j)] = a;
        }
    if constexpr (ACC) {
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double a = ::fma(Sbar, V[i], -vbar * mp[i]);
            TGP_UNROLL for (int k = 0; k < D; ++k) a = ::fma(Pp[pidx(i, k)], Vb[k], a);
            acc->gH[i] += a;
            acc->ga[i] += mb[i];
        }
        acc->gh -= vbar;
        acc->gR += Sbar;
        TGP_UNROLL for (int i = 0; i < DS; ++i) acc->gPinf[i] += Pb[i] - ad.L[i];
        const double tc = first ? 0.0 : tau, tc2 = tc * tc;      // (step 0's gap entry is a marker, not a gap)
        TGP_UNROLL for (int i = 0; i < D; ++i) {
            double ga_i = 0.0;
            const double w1 = tc * e[i], w2 = tc2 * e[i];
            TGP_UNROLL for (int k = 0; k < D; ++k) {      // G[i][k] = mb_i m_k + 2 sum_j Pb_ij (A (P - Pinf))_jk
                double a = 0.0;
                TGP_UNROLL for (int j = 0; j < D; ++j) a = ::fma(Pb[pidx(i, j)], AX[j + k * D], a);
                const double G = ::fma(2.0, a, mb[i] * xf.m[k]);
                ga_i = ::fma(G, A[i + k * D], ga_i);
                acc->gN1[i + k * D] = ::fma(w1, G, acc->gN1[i + k * D]);
                if constexpr (SdeSums<D>::LDS) sG[(D + i + k * D) * 64] = ::fma(w2, G, sG[(D + i + k * D) * 64]);
                else acc->gN2[i + k * D] = ::fma(w2, G, acc->gN2[i + k * D]);
                if (first) gA1[i + k * D] = G;
            }
            if constexpr (SdeSums<D>::LDS) sG[i * 64] = ::fma(-tc, ga_i, sG[i * 64]);
            else acc->gl[i] = ::fma(-tc, ga_i, acc->gl[i]);
        }
    }
}

// The adjoint walk of a lane over its chunk (adjoint_run's roles and layout), SDE form.
template <int D, int XS, int B, bool ACC>
TGP_HD void adjoint_run_sde(const KArgs<D>& ka, const ModelR<D, true>& mr, long long t0, int nblk, long long hi, Adj<D>& ad, AdjAccSde<D>* acc, double* sG, double* gA1,
                            double* gh_steps, double* gR_steps, const double* ckpt, double* sF, int lane, bool& ok) {
    constexpr int NS = SD<D>::NS, DS = SD<D>::DS;
    const long long T = ka.T;
    Inputs<D, true, XS, B> in, nx;
    const long long tlast = t0 + (long long)(nblk - 1) * B;
    load_inputs<D, true, XS, B>(ka, tlast, in);
    State<D> ck, ckN;
    {
        const double* q = ckpt + (size_t)(nblk > 0 ? nblk - 1 : 0) * NS * 64 + lane;
        TGP_UNROLL for (int k = 0; k < D; ++k) ck.m[k] = q[(size_t)k * 64];
        TGP_UNROLL for (int k = 0; k < DS; ++k) ck.P[k] = q[(size_t)(D + k) * 64];
    }
    for (int b = nblk - 1; b >= 0; --b) {
        const long long tb = t0 + (long long)b * B;
        load_inputs<D, true, XS, B>(ka, tb - B, nx);      // the next block (block b - 1): in flight through this one
        {
            const double* q = ckpt + (size_t)(b > 0 ? b - 1 : 0) * NS * 64 + lane;
            TGP_UNROLL for (int k = 0; k < D; ++k) ckN.m[k] = q[(size_t)k * 64];
            TGP_UNROLL for (int k = 0; k < DS; ++k) ckN.P[k] = q[(size_t)(D + k) * 64];
        }
        TGP_ISSUE_BARRIER();
        // ---- the block's filtering states, forwards from its checkpoint (the last step's is not needed: nothing walks from it)
        State<D> x = ck;
        TGP_UNROLL for (int j = 0; j + 1 < B; ++j) {
            double A[D * D];
            step_A<D, true>(ka.mc, mr, in.tau[j], tb + j == 0, A);
            predict_r<D, true>(mr, A, x.m, x.P);
            update<D>(mr.H, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, tb + j, T), x.m, x.P, (LmlAcc*)nullptr, ok);
            TGP_UNROLL for (int k = 0; k < D; ++k) sF[(j * NS + k) * 64 + lane] = x.m[k];
            TGP_UNROLL for (int k = 0; k < DS; ++k) sF[(j * NS + D + k) * 64 + lane] = x.P[k];
        }
        TGP_ISSUE_BARRIER();      // (the states are to be read back from LDS: backward_run)
        TGP_UNROLL for (int j = B - 1; j >= 0; --j) {
            const long long t = tb + j;
            if (t < hi) {
                State<D> xf = ck;
                if (j > 0) {
                    TGP_UNROLL for (int k = 0; k < D; ++k) xf.m[k] = sF[((j - 1) * NS + k) * 64 + lane];
                    TGP_UNROLL for (int k = 0; k < DS; ++k) xf.P[k] = sF[((j - 1) * NS + D + k) * 64 + lane];
                }
                double gh_t, gR_t;
                adjoint_step_sde<D, ACC>(ka.mc, mr, xf, in.tau[j], t == 0, (XS & 2) ? in.hh[j] : mr.hh, (XS & 1) ? in.R[j] : mr.R, in.y[j], in.obs(j, t, T), ad, acc,
                                         sG, gA1, gh_t, gR_t);
                if constexpr (ACC) {
                    if (gh_steps != nullptr) gh_steps[t] = gh_t;
                    if (gR_steps != nullptr) gR_steps[t] = gR_t;
                }
            }
        }
        in = nx;
        ck = ckN;
    }
}

}  // namespace tgp_sweep
