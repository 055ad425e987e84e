// A draw from the posterior of an SDE-described model on the group sweep: k_sweep_group_draw's walk and geometry (tgp_sweep_group.hip,
// DESIGN 4.12) with the transition of every step built from its gap as k_sweep_group_sde builds it (tgp_sweep_group_sde_dev.hpp).  One wave
// per workgroup, 8 groups of 8 lanes, lane j of a group holds column j of every matrix and ONE double of the sample state; 6 groups own output.
// Forwards it is forward_run_s (packed checkpoints every group_block(D) steps, no log marginal likelihood); backwards the reverse-time model's sample
// path: x_t = mf + G (x_(t+1) - mp) + chol(L + 1e-9 I).U' eps,  G = Pf A' (Pp + 1e-10 I)^-1,  L = Pf - (U G')'(U G'), where A is the transition INTO
// step t + 1 -- the gap in front of step t + 1, not step t's own.  A_t is never written, Q_t never formed: Pp = Pinf + A (Pf - Pinf) A' and A Pf, A Pinf
// apart (LaneS::predict).  tau = 0 (tied stamps) is a step with A = I that the jitters of the two factorisations carry; no branch.
// A wave's LDS is the SDE posterior kernel's: N1 and N2 (2 x 512 B), the exchange tiles and one checkpoint block of filtering states per group --
// 16 512 / 20 096 / 15 232 / 17 536 B at d = 5 / 6 / 7 / 8.  gfx950 only.
#include "tgp_sweep_group_sde_dev.hpp"

namespace tgp_sweep_group {

struct GDSArgs {
    GSArgs gs;              // (gs.ka.Wb holds the draw's warm-up Wd; mean / var unused)
    const double* eps_t;    // [T][d]: row t drives the reverse-time transition out of step t (row 0 unused)
    const double* eps_e;    // [T]
    double eps_0[G];        // the start x_(T-1)
    double* y_out;          // [T]
};
static_assert(sizeof(GDSArgs) <= 4096, "the kernel's argument segment");

template <int D, int XS> struct LaneDS : LaneS<D, XS> {
    using LaneS<D, XS>::j;
    using LaneS<D, XS>::act;
    using LaneS<D, XS>::tile;

    // Lane::draw_step with the transition of step t + 1 (s): xf = filtering state of step t, e = eps_t[t + 1]; x = x_(t+1) on entry, x_t on return.
    // Behind the predict this is that function's body, line for line, and the two must stay in step: it is repeated here, not shared, as
    // LaneS::smooth_step is -- the kernels of the other units keep their recorded resource lines.  The step does not look at the observation.
    __device__ __forceinline__ void draw_step(const StepA<D>& s, const GState<D>& xf, double& x, const double* e, bool& ok) const {
        GState<D> xp = xf;
        double AP[D];
        this->predict(s, xp, AP);      // (the filter's own predict, to the bit; A Pf and A Pinf formed separately)
        double Xc[D];
        this->gain_cols(xp.P, AP, Xc, ok);
        // ---- column j of Z = U G' from the published U (U[i][k] = tile[i + 8 k], k >= i)
        double Z[D];
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = 0.0;
            TGP_GU for (int k = i; k < D; ++k) acc = fma(tile[i + G * k], Xc[k], acc);
            Z[i] = acc;
        }
        // ---- column j of L = Pf - Z' Z: ONE publication of Z (Z[k][i] = tile[k + 8 i])
        this->publish(Z);
        double Lc[D];
        TGP_GU for (int i = 0; i < D; ++i) {
            double acc = xf.P[i];
            TGP_GU for (int k = 0; k < D; ++k) acc = fma(-tile[k + G * i], Z[k], acc);
            Lc[i] = acc;
        }
        double UL[D], rinvL[D];
        this->chol_cols(Lc, tgp_sweep::kJitterDraw, UL, rinvL, ok);
        // ---- the mean: x_j = mf_j + nz_j + sum_k G'[k][j] (x+ - mp)_k
        double dm[D];
        this->gather(x - xp.m, dm, V0);
        double acc = xf.m + this->mul_Ut(UL, e);
        TGP_GU for (int k = 0; k < D; ++k) acc = fma(Xc[k], dm[k], acc);
        x = act ? acc : 0.0;
    }
};

// the draws of the transition out of step t, one per lane of the group (lane k < d holds eps_t[t][k])
template <int D> __device__ __forceinline__ double load_eps_s(const GDSArgs& ar, long long t, int j) {
    return j < D ? ar.eps_t[(size_t)tgp_sweep::clamp_t(t, ar.gs.ka.T) * D + j] : 0.0;
}

// tgp_sweep_group.hip draw_run on the rows with the gaps.  start 0: x holds the sample of step hi (the next group's first step); 1: the run starts at
// step hi - 1 from that step's filtering mean (a warm-up); 2: from the true x_(T-1) (step hi - 1 is the series' last).  On return x is the sample of
// step t0.  The step from x_(t+1) to x_t takes the gap in FRONT of step t + 1: the next lane's of the row, or behind a row's last step the first gap of
// what lies behind it -- the next row, block or chunk (backward_run_s's tau_next; with start == 0 the first step walked, hi - 1, takes the gap of step
// hi, the next group's or wave's first).  The gap of step 0, the host's first transition, is never asked for: the walk ends at x_0.
template <int D, int XS, int B, bool EMIT>
__device__ __forceinline__ void draw_run_s(const GDSArgs& ar, const LaneDS<D, XS>& ln, long long t0, int nrows, long long hi, int start, double& x,
                                           const double* ck, size_t ck_ld, double* sF, bool& ok) {
    constexpr int NS = LaneDS<D, XS>::NS;
    const GArgs& ka = ar.gs.ka;
    RowS<XS> in, nx;
    load_row_s<XS>(ka, t0 + 8ll * (nrows - 1), ln.j, in);
    double tau_next = ka.st.tau[tgp_sweep::clamp_t(t0 + 8ll * nrows, ka.T)];
    double en = load_eps_s<D>(ar, hi, ln.j);      // what step hi - 1 consumes (unused where the run starts there)
    for (int r = nrows - 1; r >= 0; --r) {
        const long long tb = t0 + 8ll * r;
        load_row_s<XS>(ka, tb - 8, ln.j, nx);      // the next row (row r - 1): in flight through this one
        double oy = 0.0, rn = 0.0, ee = 0.0;
        if (EMIT) {
            const long long tc = tgp_sweep::clamp_t(tb + ln.j, ka.T);
            rn = ka.st.Rnew[ka.st.rnew_per_step ? tc : 0];
            ee = ar.eps_e[tc];
        }
#pragma nounroll
        for (int s = 8 / B - 1; s >= 0; --s) {
            const long long tsb = tb + s * B;
            if (tsb < hi) {
                // ---- the block's filtering states, forwards from its checkpoint
                GState<D> xw;
                ln.load_packed(ck + (size_t)((tsb - t0) / B) * ck_ld, xw);
                wave_sync();
#pragma nounroll
                for (int k = 0; k < B; ++k) {
                    ln.fstep(xw, in, s * B + k, tsb + k, ka.T, (LmlAcc*)nullptr, ok);
                    ln.store_packed(sF + k * NS, xw);
                }
                wave_sync();
                // ---- backwards through the block
#pragma nounroll
                for (int k = B - 1; k >= 0; --k) {
                    const long long t = tsb + k;
                    if (t < hi) {
                        const int q = s * B + k;
                        GState<D> xf;
                        ln.load_packed(sF + k * NS, xf);
                        const double ec = en;
                        en = load_eps_s<D>(ar, t, ln.j);      // step t - 1's draws: in flight through this step
                        double e[D];
                        if (start != 0 && t == hi - 1) {
                            if (start == 2) {
                                TGP_GU for (int i = 0; i < D; ++i) e[i] = ar.eps_0[i];
                                x = ln.draw_start(xf, e, ok);
                            } else {
                                x = xf.m;
                            }
                        } else {
                            TGP_GU for (int i = 0; i < D; ++i) e[i] = __shfl(ec, i, G);
                            const double tn = __shfl(in.tau, (q + 1) & 7, G);
                            StepA<D> sa;
                            ln.step_A(q == 7 ? tau_next : tn, sa);
                            ln.draw_step(sa, xf, x, e, ok);
                        }
                        if (EMIT) {
                            const double hx = group_sum(ln.Hj * x) + ((XS & 2) ? __shfl(in.hh, q, G) : ln.hh);
                            oy = (ln.j == q) ? hx : oy;
                        }
                    }
                }
            }
        }
        if (EMIT && tb + ln.j < hi) ar.y_out[tb + ln.j] = fma(::sqrt(rn), ee, oy);
        tau_next = __shfl(in.tau, 0, G);
        in = nx;
    }
}

// part[wave]: [0, bits, dist_f, dist_d].  The register counts are in profiles/sweep_group_draw_sde_resources.txt.
template <int D, int XS>
__global__ __launch_bounds__(64) void k_sweep_group_draw_sde(const GDSArgs by_value) {
    (void)by_value;
    const GDSArgs& ar = *(const GDSArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place: tgp_sweep.hip k_sweep)
    const GArgs& ka = ar.gs.ka;
    constexpr int B = tgp_sweep::group_block(D), NS = LaneDS<D, XS>::NS, NG = tgp_sweep::kGroupsPerWave;
    __shared__ __attribute__((aligned(16))) double sN[2 * G * G];
    __shared__ double tiles[NG * kTileLD];
    __shared__ double sF[NG * B * NS];
    const int lane = threadIdx.x, g = lane / G;
    const long long wave = blockIdx.x;
    sN[lane] = ar.gs.sc.N1[lane];
    sN[G * G + lane] = ar.gs.sc.N2[lane];
    __syncthreads();

    LaneDS<D, XS> ln;
    ln.j = lane % G;
    ln.act = ln.j < D;
    ln.tile = tiles + g * kTileLD;
    ln.sA = nullptr;
    ln.sN1 = sN;
    ln.sN2 = sN + G * G;
    const int j = ln.j;
    TGP_GU for (int i = 0; i < D; ++i) {
        ln.Gc[i] = ln.act ? ka.mc.gP[i + G * j] : 0.0;
        ln.lam[i] = ar.gs.sc.lam[i];
        ln.H[i] = ka.mc.H[i];
    }
    ln.Hj = ln.act ? ka.mc.H[j] : 0.0;
    ln.aj = ln.act ? ka.mc.a[j] : 0.0;
    ln.hh = ka.mc.hh;
    ln.R = ka.mc.R;

    const long long T = ka.T;
    const int C = ka.C;
    const tgp_sweep::GroupSpan span = tgp_sweep::group_span(wave, g, ka.owned, ka.nchunks, C, T);
    const long long t0 = span.t0, t1 = span.t1;
    const long long t1r = (t1 + 7) & ~7ll;
    const bool runs = span.runs;          // group 0 only warms up for group 1
    const bool owned = span.owned;        // group 7 only warms up backwards for group 6
    bool ok = true;

    GState<D> gen, x0;      // gen: (x0m, Pinf), where a warm-up starts from; x0: the state in front of update 0
    gen.m = ln.act ? ka.mc.gm[j] : 0.0;
    x0.m = ln.act ? ka.mc.x0m[j] : 0.0;
    TGP_GU for (int i = 0; i < D; ++i) {
        gen.P[i] = ln.Gc[i];
        x0.P[i] = ln.act ? ka.mc.x0P[i + G * j] : 0.0;
    }
    const size_t ck_ld = (size_t)NG * NS;
    double* ck = ka.ckpt + (size_t)wave * (size_t)(C / B) * ck_ld + (size_t)g * NS;
    double* sFg = sF + g * B * NS;

    // ---- forwards: k_sweep_group_sde<POST>'s two passes (warm-up, hand-over, the chunk with its checkpoints); no log marginal likelihood
    GState<D> x, e1;
    {
        LmlAcc acc;
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        forward_run_s<D, XS, B>(ka, ln, tw, ka.W / 8, tw > 0 ? tw : 0, t1r, x, acc, false, (double*)nullptr, 0, 0, ok);
        e1 = x;
        x.m = __shfl_up(e1.m, G, 64);
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] = __shfl_up(e1.P[i], G, 64);
        if (t0 == 0) x = x0;
        forward_run_s<D, XS, B>(ka, ln, t0, C / 8, t0, runs ? t1r : t0, x, acc, false, ck, t0, ck_ld, ok);
    }
    double dist_f = 0.0, dist_d = 0.0;
    bool finite = true;
    {
        const double df = ln.distance(ka.mc, x, e1);
        const bool fin = ln.finite(x) && ln.finite(e1);
        if (owned) {
            dist_f = df;
            finite = fin;
        }
    }

    // ---- backwards, the warm-up: the sample of the chunk's first step as the walk over its first Wd steps gives it from the filtering mean behind them,
    // with the real draws (exact where they reach the series' last step: the true x_(T-1)) -- what the PREVIOUS group continues from
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // (the checkpoints are read back by other lanes of the group)
    double b1 = 0.0;
    {
        const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
        draw_run_s<D, XS, B, false>(ar, ln, t0, ka.Wb / 8, runs ? te : t0, te == T ? 2 : 1, b1, ck, ck_ld, sFg, ok);
    }
    // ---- backwards, the chunk: from the next group's sample of ITS first step; y* of every step
    double xs = __shfl_down(b1, G, 64);
    draw_run_s<D, XS, B, true>(ar, ln, t0, C / 8, owned ? t1 : t0, t1 == T ? 2 : 0, xs, ck, ck_ld, sFg, ok);
    {
        const double dd = ln.draw_distance(ka.mc, xs, b1);
        const bool fin = group_sum(::fabs(xs) + ::fabs(b1)) < 1e300;
        if (owned) {
            dist_d = dd;
            finite = finite && fin;
        }
    }

    unsigned bits = 0;
    if (owned && !(dist_f <= ka.mc.tol)) bits |= 1u;
    if (owned && !(dist_d <= ka.mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
        const double of = __shfl_xor(dist_f, off, 64), ob = __shfl_xor(dist_d, off, 64);
        dist_f = (of > dist_f) ? of : dist_f;
        dist_d = (ob > dist_d) ? ob : dist_d;
    }
    if (lane == 0) {
        double* p = ka.part + (size_t)wave * 4;
        p[0] = 0.0;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_d;
    }
}

namespace {

template <int D> void launch_d(unsigned nwaves, hipStream_t stream, const GDSArgs& ar) {
    const dim3 grid(nwaves), block(64);
    const int xs = (ar.gs.ka.st.R != nullptr ? 1 : 0) | (ar.gs.ka.st.hh != nullptr ? 2 : 0);
    switch (xs) {
        case 0: hipLaunchKernelGGL((k_sweep_group_draw_sde<D, 0>), grid, block, 0, stream, ar); break;
        case 1: hipLaunchKernelGGL((k_sweep_group_draw_sde<D, 1>), grid, block, 0, stream, ar); break;
        case 2: hipLaunchKernelGGL((k_sweep_group_draw_sde<D, 2>), grid, block, 0, stream, ar); break;
        default: hipLaunchKernelGGL((k_sweep_group_draw_sde<D, 3>), grid, block, 0, stream, ar); break;
    }
}

}  // namespace

void launch_draw_sde(int d, unsigned nwaves, hipStream_t stream, const GArgs& ka, const tgp_sweep::GroupSdeC& sc, const double* eps_t, const double* eps_e,
                     const double* eps_0, double* y_out) {
    GDSArgs ar;
    ar.gs.ka = ka;
    ar.gs.sc = sc;
    ar.eps_t = eps_t;
    ar.eps_e = eps_e;
    for (int k = 0; k < G; ++k) ar.eps_0[k] = k < d ? eps_0[k] : 0.0;
    ar.y_out = y_out;
    switch (d) {
        case 5: launch_d<5>(nwaves, stream, ar); break;
        case 6: launch_d<6>(nwaves, stream, ar); break;
        case 7: launch_d<7>(nwaves, stream, ar); break;
        default: launch_d<8>(nwaves, stream, ar); break;
    }
}

}  // namespace tgp_sweep_group
