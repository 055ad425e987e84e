// TEST INFRASTRUCTURE ONLY (never part of the product library, never a fallback).
// The sweep engine's adjoint gradient for SDE-described models (temporalgps.jl_amd/csrc/tgp_sweep.hip k_sweep_adjoint_sde) run on the host: the
// product's own plan (tgp_sweep_plan.hpp) and the very functions its kernel calls per lane (tgp_sweep_body.hpp: forward_run, adjoint_run_sde,
// adjoint_step_sde, adjoint_distance), with the wave's 64 lanes visited one after the other and the two cross-lane shifts done by hand.
// What is NOT exercised here is k_sweep_adjoint_sde's own orchestration, which this file restates as sweepadjsim.cpp restates k_sweep_adjoint's; the
// GPU tier covers it.
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../temporalgps.jl_amd/csrc/tgp_sweep_plan.hpp"

using namespace tgp_sweep;

namespace {

template <int D> bool finite_state(const State<D>& x) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += std::fabs(x.m[k]);
    for (int k = 0; k < SD<D>::DS; ++k) s += std::fabs(x.P[k]);
    return s < 1e300;
}
template <int D> bool finite_adj(const Adj<D>& x) {
    double s = 0.0;
    for (int k = 0; k < D; ++k) s += std::fabs(x.l[k]);
    for (int k = 0; k < SD<D>::DS; ++k) s += std::fabs(x.L[k]);
    return s < 1e300;
}

// g: [gl d | gN1 d*d | gN2 d*d | gPinf d*d | ga d | gH d | gh | gR | gA1 d*d | gx0m d | gx0P d*d], column-major blocks
template <int D, int XS> void run_d(const Plan& p, const Streams& st, double* gh_steps, double* gR_steps, double* g, double* out) {
    constexpr int B = SdeSums<D>::B, NS = SD<D>::NS, DS = SD<D>::DS;
    KArgs<D> ka;
    std::memcpy(&ka.mc, p.mc, sizeof ka.mc);
    ka.st = st;
    ka.T = p.T;
    ka.C = p.C;
    ka.W = p.W;
    ka.Wb = p.Wa;      // (the kernel's second warm-up is the adjoint's)
    ka.nchunks = p.nchunks;
    ka.mean = nullptr;
    ka.var = nullptr;
    const int C = p.C;
    const long long T = p.T;
    std::vector<double> ckpt((size_t)(C / B) * NS * 64), sF((size_t)B * NS * 64);
    double lml = 0.0, dfw = 0.0, dbw = 0.0;
    unsigned bits_total = 0;
    ModelR<D, true> mr;
    mr.init(ka.mc);
    State<D> gen, x0;
    set_state<D>(gen, ka.mc.gm, ka.mc.gP);
    set_state<D>(x0, ka.mc.x0m, ka.mc.x0P);
    AdjAccSde<D> tot;
    tot.zero();
    double gA1[D * D] = {};
    std::vector<double> sS((size_t)SdeSums<D>::NL * 64);      // the lanes' gl and gN2 sums where the kernel keeps them in LDS
    Adj<D> gx0;
    gx0.zero();
    for (long long wave = 0; wave < p.nwaves; ++wave) {
        long long t0[64], t1[64], t1r[64];
        bool runs[64], owned[64], ok[64];
        State<D> e1[64], x[64];
        Adj<D> b1[64];
        LmlAcc acc[64];
        for (int lane = 0; lane < 64; ++lane) {
            const long long c = wave * kOwned + lane - 1;
            const bool active = c >= 0 && c < p.nchunks;
            t0[lane] = active ? c * C : 0;
            long long e = active ? t0[lane] + C : 0;
            t1[lane] = e < T ? e : (active ? T : 0);
            t1r[lane] = (t1[lane] + 7) & ~7ll;
            runs[lane] = active && lane >= 1;
            owned[lane] = runs[lane] && lane <= kOwned;
            ok[lane] = true;
        }
        for (int lane = 0; lane < 64; ++lane) {
            const long long tw = t1r[lane] - ka.W;
            State<D> s = tw <= 0 ? x0 : gen;
            LmlAcc dummy;
            forward_run<D, true, XS, B>(ka, mr, tw, ka.W / B, tw > 0 ? tw : 0, t1r[lane], s, dummy, false, (double*)nullptr, lane, ok[lane]);
            e1[lane] = s;
        }
        for (int lane = 0; lane < 64; ++lane) {
            x[lane] = lane > 0 ? e1[lane - 1] : e1[0];
            if (t0[lane] == 0) x[lane] = x0;
            forward_run<D, true, XS, B>(ka, mr, t0[lane], C / B, t0[lane], runs[lane] ? t1r[lane] : t0[lane], x[lane], acc[lane], true, ckpt.data(), lane, ok[lane]);
        }
        double df[64] = {}, db[64] = {};
        bool fin[64];
        for (int lane = 0; lane < 64; ++lane) {
            fin[lane] = true;
            if (owned[lane]) {
                df[lane] = state_distance<D>(ka.mc, x[lane], e1[lane]);
                fin[lane] = finite_state<D>(x[lane]) && finite_state<D>(e1[lane]);
            }
        }
        // backwards, the warm-up: the chunk's first Wa steps from a zero adjoint, nothing summed
        for (int lane = 0; lane < 64; ++lane) {
            const long long te = (t0[lane] + ka.Wb < t1[lane]) ? t0[lane] + ka.Wb : t1[lane];
            b1[lane].zero();
            adjoint_run_sde<D, XS, B, false>(ka, mr, t0[lane], ka.Wb / B, runs[lane] ? te : t0[lane], b1[lane], (AdjAccSde<D>*)nullptr, nullptr, nullptr, nullptr, nullptr,
                                             ckpt.data(), sF.data(), lane, ok[lane]);
        }
        // the shift; the chunk from the next lane's adjoint in front of ITS first step
        for (int lane = 0; lane < 64; ++lane) {
            Adj<D> ad = lane < 63 ? b1[lane + 1] : b1[63];
            if (t1[lane] == T) ad.zero();
            AdjAccSde<D> ga;
            ga.zero();
            for (int k = 0; k < SdeSums<D>::NL; ++k) sS[(size_t)k * 64 + lane] = 0.0;
            adjoint_run_sde<D, XS, B, true>(ka, mr, t0[lane], C / B, owned[lane] ? t1[lane] : t0[lane], ad, &ga, sS.data() + lane, gA1, gh_steps, gR_steps, ckpt.data(),
                                            sF.data(), lane, ok[lane]);
            if (SdeSums<D>::LDS) {
                for (int i = 0; i < D; ++i) ga.gl[i] = sS[(size_t)i * 64 + lane];
                for (int i = 0; i < D * D; ++i) ga.gN2[i] = sS[(size_t)(D + i) * 64 + lane];
            }
            if (owned[lane]) {
                db[lane] = adjoint_distance<D>(ka.mc, ad, b1[lane]);
                fin[lane] = fin[lane] && finite_adj<D>(ad) && finite_adj<D>(b1[lane]);
                lml += acc[lane].total();
                for (int i = 0; i < D * D; ++i) { tot.gN1[i] += ga.gN1[i]; tot.gN2[i] += ga.gN2[i]; }
                for (int i = 0; i < D; ++i) { tot.gl[i] += ga.gl[i]; tot.ga[i] += ga.ga[i]; tot.gH[i] += ga.gH[i]; }
                for (int i = 0; i < DS; ++i) tot.gPinf[i] += ga.gPinf[i];
                tot.gh += ga.gh;
                tot.gR += ga.gR;
                if (wave * kOwned + lane - 1 == 0) gx0 = ad;
            }
        }
        unsigned bits = 0;
        for (int lane = 0; lane < 64; ++lane) {
            if (owned[lane] && !(df[lane] <= ka.mc.tol)) bits |= 1u;
            if (owned[lane] && !(db[lane] <= ka.mc.tol_b)) bits |= 2u;
            if (!ok[lane]) bits |= 4u;
            if (!fin[lane]) bits |= 8u;
            dfw = std::max(dfw, df[lane]);
            dbw = std::max(dbw, db[lane]);
        }
        bits_total |= bits;
    }
    double* q = g;
    for (int i = 0; i < D; ++i) *q++ = tot.gl[i];
    for (int i = 0; i < D * D; ++i) *q++ = tot.gN1[i];
    for (int i = 0; i < D * D; ++i) *q++ = tot.gN2[i];
    for (int j = 0; j < D; ++j) for (int i = 0; i < D; ++i) *q++ = tot.gPinf[pidx(i, j)];
    for (int i = 0; i < D; ++i) *q++ = tot.ga[i];
    for (int i = 0; i < D; ++i) *q++ = tot.gH[i];
    *q++ = tot.gh;
    *q++ = tot.gR;
    for (int i = 0; i < D * D; ++i) *q++ = gA1[i];
    for (int i = 0; i < D; ++i) *q++ = gx0.l[i];
    for (int j = 0; j < D; ++j) for (int i = 0; i < D; ++i) *q++ = gx0.L[pidx(i, j)];
    out[0] = lml;
    out[1] = (double)bits_total;
    out[2] = dfw;
    out[3] = dbw;
}

template <int D> void run_x(const Plan& p, const Streams& st, double* gh_steps, double* gR_steps, double* g, double* out) {
    switch ((st.R != nullptr ? 1 : 0) | (st.hh != nullptr ? 2 : 0)) {
        case 0: run_d<D, 0>(p, st, gh_steps, gR_steps, g, out); break;
        case 1: run_d<D, 1>(p, st, gh_steps, gR_steps, g, out); break;
        case 2: run_d<D, 2>(p, st, gh_steps, gR_steps, g, out); break;
        default: run_d<D, 3>(p, st, gh_steps, gR_steps, g, out); break;
    }
}

}  // namespace

extern "C" int sweepadjsdesim_run(int d, int64_t T, const double* A1, const double* a, const double* Q1, const double* H, double hh, double R, const double* x0m,
                                  const double* x0P, const double* Pinf, const double* coef, double tau_typ, const double* y, const uint8_t* mask,
                                  const double* Rstep, const double* hstep, const double* tau, int fC, int fW, int fWa, int w_hint, int wa_hint, int num_cu,
                                  double* gh_steps, double* gR_steps, double* g, double* out) {
    ModelHost m;
    m.d = d;
    m.sde = true;
    m.A = A1; m.a = a; m.Q = Q1; m.H = H; m.hh = hh; m.R = R; m.x0m = x0m; m.x0P = x0P; m.Pinf = Pinf; m.coef = coef; m.tau_typ = tau_typ;
    Plan p;
    Forced f;
    f.C = fC; f.W = fW; f.Wa = fWa;
    std::string why;
    if (!make_plan(&p, f, m, T, w_hint, 0, num_cu, &why, 0, wa_hint)) return 1;
    Streams st;
    st.y = y; st.mask = mask; st.R = Rstep; st.hh = hstep; st.tau = tau;
    switch (d) {
        case 1: run_x<1>(p, st, gh_steps, gR_steps, g, out); break;
        case 2: run_x<2>(p, st, gh_steps, gR_steps, g, out); break;
        case 3: run_x<3>(p, st, gh_steps, gR_steps, g, out); break;
        default: run_x<4>(p, st, gh_steps, gR_steps, g, out); break;
    }
    out[4] = p.C;
    out[5] = p.W;
    out[6] = p.Wa;
    out[7] = (double)p.nwaves;
    return 0;
}
