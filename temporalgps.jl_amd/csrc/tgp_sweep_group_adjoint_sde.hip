// The adjoint gradient of the group sweep on SDE-described models: k_sweep_group_adjoint's walk and geometry (tgp_sweep_group.hip)
// with the transition of every step built from its gap as k_sweep_group_sde builds it (tgp_sweep_group_sde_dev.hpp), and the mathematics of
// k_sweep_adjoint_sde (tgp_sweep_body.hpp adjoint_step_sde) in the column layout: lane j of a group holds l_j and column j of the symmetric L.
// G_t = d logpdf / d A_t = mb m' + 2 Pb A_t (P - Pinf) is never stored: a lane contracts ITS column of it on the spot into sums over the closed form's
// coefficients -- row i of gl, gN1[:, j], gN2[:, j] -- and Pinf collects Pb - A_t' Pb A_t.  A_t is never stored either: its column j and the products with
// A_t' are formed from N1 / N2 in LDS and the step's exponentials.
// The kernel never sees the series' first transition (the host has predicted the prior through it): at t == 0 the step is the update alone, and the group
// that owns chunk 0 leaves the adjoint in FRONT of update 0, which the host pulls back through A1 (tgp_sweep_group.hip adjoint_blocks_sde).
// A wave's LDS is the posterior call's: N1 and N2, the exchange tiles and one checkpoint block of states per group.  gfx950 only.
#include "tgp_sweep_group_sde_dev.hpp"

namespace tgp_sweep_group {

struct GASArgs {
    GSArgs gs;             // (gs.ka.Wb holds the adjoint's warm-up Wa; mean / var unused)
    double* gh_steps;      // [T] or null: d logpdf / d h_t, d logpdf / d R_t of every step
    double* gR_steps;
};
static_assert(sizeof(GASArgs) <= 4096, "the kernel's argument segment");

// a lane's sums over the steps of its group's chunk: column j of gN1, gN2 and gPinf, its column's share of every row of gl (summed over the lanes of the
// group at the end), element j of ga and gH, the sums of the per-step gh_t and gR_t (the same in every lane of the group)
template <int D> struct GAccS {
    double gl[D], gN1[D], gN2[D], gPi[D], ga, gH, gh, gR;
    __device__ __forceinline__ void zero() {
        TGP_GU for (int i = 0; i < D; ++i) gl[i] = gN1[i] = gN2[i] = gPi[i] = 0.0;
        ga = gH = gh = gR = 0.0;
    }
};

template <int D, int XS> struct LaneAS : LaneS<D, XS> {
    using LaneS<D, XS>::j;
    using LaneS<D, XS>::tile;
    using LaneS<D, XS>::H;
    using LaneS<D, XS>::sN1;
    using LaneS<D, XS>::sN2;
    using LaneS<D, XS>::Gc;

    // One step backwards (Lane::adjoint_step's roles).  s: the transition of step t (tau = 0 at t == 0); first: t == 0 -- the state in front of the step
    // is the host's prediction and is kept; with tau = 0 the transition is the identity to the bit, so `ad` returns as the adjoint in front of the UPDATE,
    // nothing reaches the coefficient sums or gPinf, and ga alone needs a select.  Behind the predict the update's adjoint is Lane::adjoint_step's, line
    // for line (repeated, not shared: that function's kernels keep their recorded resource lines).
    template <bool ACC>
    __device__ __forceinline__ void adjoint_step(const StepA<D>& s, bool first, const GState<D>& xf, double y, double Rt, double ht, bool obs, GState<D>& ad,
                                                 GAccS<D>* acc, double& gh_t, double& gR_t) const {
        double AD[D];      // column j of A_t (P - Pinf): what LaneS::predict sends through the tile
        {
            double Dc[D];
            TGP_GU for (int i = 0; i < D; ++i) Dc[i] = xf.P[i] - Gc[i];
            this->mul_A(s, Dc, AD);
        }
        GState<D> xp = xf;
        this->predict(s, xp);      // (the filter's own predict, to the bit)
        if (first) xp = xf;
        double vj = 0.0;      // V = Pp H, element j
        TGP_GU for (int i = 0; i < D; ++i) vj = fma(xp.P[i], H[i], vj);
        const double s2 = group_sum(this->Hj * vj) + Rt;
        const double hm = group_sum(this->Hj * xp.m) + ht;
        const double S = obs ? s2 : 1.0;
        const double iS = obs ? fast_rcp(S) : 0.0;      // (a missing step: every term of the update's adjoint below is a multiple of iS or v)
        const double v = obs ? (y - hm) : 0.0;
        const double viS = v * iS;
        double V[D];
        this->gather(vj, V, V1);
        double lvj = 0.0;      // (L V)_j: lane-local by symmetry
        TGP_GU for (int i = 0; i < D; ++i) lvj = fma(ad.P[i], V[i], lvj);
        const double lV = group_sum(ad.m * vj);
        const double VLV = group_sum(vj * lvj);
        const double vbar = (lV - v) * iS;
        const double Sbar = fma(fma(-lV, v, VLV) * iS, iS, -0.5 * fma(-viS, viS, iS));
        const double vbj = fma(Sbar, this->Hj, fma(ad.m, viS, -2.0 * iS * lvj));
        gh_t = -vbar;
        gR_t = Sbar;
        double Vb[D];
        this->gather(vbj, Vb, V0);
        const double mbj = fma(-vbar, this->Hj, ad.m);
        double Pb[D];      // column j of Pb = L + (Vb H' + H Vb') / 2
        TGP_GU for (int i = 0; i < D; ++i) Pb[i] = fma(0.5, fma(Vb[i], this->Hj, H[i] * vbj), ad.P[i]);
        if (ACC) {
            double a = fma(Sbar, vj, -vbar * xp.m);
            TGP_GU for (int i = 0; i < D; ++i) a = fma(xp.P[i], Vb[i], a);
            acc->gH += a;
            acc->ga += first ? 0.0 : mbj;      // (step 0's share belongs to the host's pull-back through A1)
            acc->gh -= vbar;
            acc->gR += Sbar;
        }
        // Pb and mb through the tile, ONE trip; everything behind it is lane-local
        wave_sync();
        TGP_GU for (int i = 0; i < D; ++i) tile[i + G * j] = Pb[i];
        tile[V0 + j] = mbj;
        wave_sync();
        double mb[D], Ac[D], u[D], w[D];
        TGP_GU for (int k = 0; k < D; ++k) {
            mb[k] = tile[V0 + k];
            // column j of A_t (zero in a padding lane and outside the band: N1 and N2 are zero there)
            Ac[k] = s.e[k] * fma(s.tau, fma(s.tau, sN2[G * k + j], sN1[G * k + j]), (k == j) ? 1.0 : 0.0);
        }
        TGP_GU for (int i = 0; i < D; ++i) {
            double au = 0.0, aw = 0.0;
            TGP_GU for (int k = 0; k < D; ++k) {
                const double p = tile[i + G * k];
                if (ACC) au = fma(p, AD[k], au);
                aw = fma(p, Ac[k], aw);
            }
            u[i] = au;
            w[i] = aw;
        }
        if (ACC) {      // G_t[:, j] = mb m_j + 2 Pb AD[:, j], contracted: gl_i -= tau G_ij A_ij, gN1_ij += tau e_i G_ij, gN2_ij += tau^2 e_i G_ij
            TGP_GU for (int i = 0; i < D; ++i) {
                const double g = fma(2.0, u[i], mb[i] * xf.m);
                const double te = s.tau * s.e[i];
                acc->gl[i] = fma(-s.tau * Ac[i], g, acc->gl[i]);
                acc->gN1[i] = fma(te, g, acc->gN1[i]);
                acc->gN2[i] = fma(te * s.tau, g, acc->gN2[i]);
            }
        }
        // l <- A_t' mb, element j;  L <- A_t' Pb A_t, column j = A_t' w: (A_t' w)_i = (e w)_i + tau (N1' (e w))_i + tau^2 (N2' (e w))_i over the band
        double al = 0.0;
        TGP_GU for (int k = 0; k < D; ++k) {
            al = fma(Ac[k], mb[k], al);
            w[k] *= s.e[k];
        }
        ad.m = al;
        TGP_GU for (int i = 0; i < D; ++i) {
            double a1 = 0.0, a2 = 0.0;
            TGP_GU for (int k = (i > kBand ? i - kBand : 0); k <= (i + kBand < D - 1 ? i + kBand : D - 1); ++k) {
                a1 = fma(sN1[G * k + i], w[k], a1);
                a2 = fma(sN2[G * k + i], w[k], a2);
            }
            const double ln = fma(s.tau, fma(s.tau, a2, a1), w[i]);
            if (ACC) acc->gPi[i] += Pb[i] - ln;
            ad.P[i] = ln;
        }
    }
};

// tgp_sweep_group.hip adjoint_run with the gaps in the rows: the step in front of t needs the gap of step t alone (the adjoint step reads the state in
// FRONT of step t and applies A_t)
template <int D, int XS, int B, bool ACC>
__device__ __forceinline__ void adjoint_run_s(const GArgs& ka, const LaneAS<D, XS>& ln, long long t0, int nrows, long long hi, GState<D>& ad, GAccS<D>* acc,
                                              double* gh_steps, double* gR_steps, const double* ck, size_t ck_ld, double* sF, bool& ok) {
    constexpr int NS = LaneAS<D, XS>::NS;
    RowS<XS> in, nx;
    load_row_s<XS>(ka, t0 + 8ll * (nrows - 1), ln.j, in);
    for (int r = nrows - 1; r >= 0; --r) {
        const long long tb = t0 + 8ll * r;
        load_row_s<XS>(ka, tb - 8, ln.j, nx);      // the next row (row r - 1): in flight through this one
        double og = 0.0, oR = 0.0;
#pragma nounroll
        for (int s = 8 / B - 1; s >= 0; --s) {
            const long long tsb = tb + s * B;
            if (tsb < hi) {
                // ---- the states in front of the block's steps, forwards from its checkpoint
                GState<D> x;
                ln.load_packed(ck + (size_t)((tsb - t0) / B) * ck_ld, x);
                wave_sync();
                ln.store_packed(sF, x);
#pragma nounroll
                for (int k = 0; k + 1 < B; ++k) {
                    ln.fstep(x, in, s * B + k, tsb + k, ka.T, (LmlAcc*)nullptr, ok);
                    ln.store_packed(sF + (k + 1) * NS, x);
                }
                wave_sync();
                // ---- backwards through the block
#pragma nounroll
                for (int k = B - 1; k >= 0; --k) {
                    const long long t = tsb + k;
                    if (t < hi) {
                        GState<D> xf;
                        ln.load_packed(sF + k * NS, xf);
                        const int q = s * B + k;
                        const double y = __shfl(in.y, q, G);
                        const double Rt = (XS & 1) ? __shfl(in.R, q, G) : ln.R;
                        const double ht = (XS & 2) ? __shfl(in.hh, q, G) : ln.hh;
                        const bool obs = t < ka.T && __shfl((int)in.mk, q, G) == 0;
                        const double tau = __shfl(in.tau, q, G);
                        StepA<D> sa;
                        ln.step_A(t <= 0 ? 0.0 : tau, sa);
                        double gh_t, gR_t;
                        ln.template adjoint_step<ACC>(sa, t == 0, xf, y, Rt, ht, obs, ad, acc, gh_t, gR_t);
                        og = (ln.j == q) ? gh_t : og;
                        oR = (ln.j == q) ? gR_t : oR;
                    }
                }
            }
        }
        if (ACC && tb + ln.j < hi) {
            if (gh_steps != nullptr) gh_steps[tb + ln.j] = og;
            if (gR_steps != nullptr) gR_steps[tb + ln.j] = oR;
        }
        in = nx;
    }
}

// part[wave]: [lml, bits, dist_f, dist_b | gl d | gN1 d*d | gN2 d*d | gPinf packed | ga d | gH d | sum gh_t | sum gR_t | mb_0 d | Pb_0 packed]
// (tgp_sweep_plan.hpp group_adjoint_sde_sums; (mb_0, Pb_0): the adjoint in front of update 0).  The register counts are in
// profiles/sweep_group_adjoint_sde_resources.txt.
template <int D, int XS>
__global__ __launch_bounds__(64) void k_sweep_group_adjoint_sde(const GASArgs by_value) {
    (void)by_value;
    const GASArgs& ar = *(const GASArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place: tgp_sweep.hip k_sweep)
    const GArgs& ka = ar.gs.ka;
    constexpr int B = tgp_sweep::group_block(D), NS = LaneAS<D, XS>::NS, DS = D * (D + 1) / 2, NG = tgp_sweep::kGroupsPerWave;
    __shared__ __attribute__((aligned(16))) double sN[2 * G * G];
    __shared__ double tiles[NG * kTileLD];
    __shared__ double sF[NG * B * NS];
    const int lane = threadIdx.x, g = lane / G;
    const long long wave = blockIdx.x;
    sN[lane] = ar.gs.sc.N1[lane];
    sN[G * G + lane] = ar.gs.sc.N2[lane];
    __syncthreads();

    LaneAS<D, XS> ln;
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

    // ---- forwards: k_sweep_group_sde<POST>'s two passes (warm-up, hand-over, the chunk with its checkpoints and the log marginal likelihood)
    GState<D> x, e1;
    LmlAcc acc;
    {
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        forward_run_s<D, XS, B>(ka, ln, tw, ka.W / 8, tw > 0 ? tw : 0, t1r, x, acc, false, (double*)nullptr, 0, 0, ok);
        e1 = x;
        x.m = __shfl_up(e1.m, G, 64);
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] = __shfl_up(e1.P[i], G, 64);
        if (t0 == 0) x = x0;
        acc = LmlAcc();
        forward_run_s<D, XS, B>(ka, ln, t0, C / 8, t0, runs ? t1r : t0, x, acc, true, ck, t0, ck_ld, ok);
    }
    double dist_f = 0.0, dist_b = 0.0;
    bool finite = true;
    {
        const double df = ln.distance(ka.mc, x, e1);
        const bool fin = ln.finite(x) && ln.finite(e1);
        if (owned) {
            dist_f = df;
            finite = fin;
        }
    }

    // ---- backwards, the warm-up: the adjoint in front of the chunk's first step as its first Wa steps give it from zero (exact where they reach the
    // series' last step) -- what the PREVIOUS group continues from
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // (the checkpoints are read back by other lanes of the group)
    GState<D> b1;
    b1.m = 0.0;
    TGP_GU for (int i = 0; i < D; ++i) b1.P[i] = 0.0;
    {
        const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
        adjoint_run_s<D, XS, B, false>(ka, ln, t0, ka.Wb / 8, runs ? te : t0, b1, (GAccS<D>*)nullptr, (double*)nullptr, (double*)nullptr, ck, ck_ld, sFg, ok);
    }
    // ---- backwards, the chunk: from the next group's adjoint in front of ITS first step (zero behind the series' last step)
    GState<D> ad;
    ad.m = __shfl_down(b1.m, G, 64);
    TGP_GU for (int i = 0; i < D; ++i) ad.P[i] = __shfl_down(b1.P[i], G, 64);
    if (t1 == T) {
        ad.m = 0.0;
        TGP_GU for (int i = 0; i < D; ++i) ad.P[i] = 0.0;
    }
    GAccS<D> ga;
    ga.zero();
    adjoint_run_s<D, XS, B, true>(ka, ln, t0, C / 8, owned ? t1 : t0, ad, &ga, ar.gh_steps, ar.gR_steps, ck, ck_ld, sFg, ok);
    {
        const double db = ln.adjoint_distance(ka.mc, ad, b1);
        const bool fin = ln.finite(ad) && ln.finite(b1);
        if (owned) {
            dist_b = db;
            finite = finite && fin;
        }
    }

    // ---- the wave's share: the groups' sums added in a fixed order (lane j of every group holds column j), gl's rows over the lanes of a group behind
    // that, then lanes 0 .. d - 1 write their columns
    const bool first = owned && span.t0 == 0;      // the adjoint in front of update 0: the host pulls it back through the first transition
    double gxm = first ? ad.m : 0.0, gxP[D];
    TGP_GU for (int i = 0; i < D; ++i) gxP[i] = first ? ad.P[i] : 0.0;
    {
        double s = ::fabs(ga.ga) + ::fabs(ga.gH) + ::fabs(ga.gh) + ::fabs(ga.gR);
        TGP_GU for (int i = 0; i < D; ++i) s += ::fabs(ga.gl[i]) + ::fabs(ga.gN1[i]) + ::fabs(ga.gN2[i]) + ::fabs(ga.gPi[i]);
        finite = finite && (s < 1e300);
    }
    double lml = (owned && j == 0) ? acc.total() : 0.0;
    finite = finite && (::fabs(lml) < 1e300);
    unsigned bits = 0;
    if (owned && !(dist_f <= ka.mc.tol)) bits |= 1u;
    if (owned && !(dist_b <= ka.mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
#pragma unroll
    for (int off = 8; off <= 32; off <<= 1) {
        TGP_GU for (int i = 0; i < D; ++i) {
            ga.gl[i] += __shfl_xor(ga.gl[i], off, 64);
            ga.gN1[i] += __shfl_xor(ga.gN1[i], off, 64);
            ga.gN2[i] += __shfl_xor(ga.gN2[i], off, 64);
            ga.gPi[i] += __shfl_xor(ga.gPi[i], off, 64);
            gxP[i] += __shfl_xor(gxP[i], off, 64);
        }
        ga.ga += __shfl_xor(ga.ga, off, 64);
        ga.gH += __shfl_xor(ga.gH, off, 64);
        ga.gh += __shfl_xor(ga.gh, off, 64);
        ga.gR += __shfl_xor(ga.gR, off, 64);
        gxm += __shfl_xor(gxm, off, 64);
    }
#pragma unroll
    for (int off = 1; off <= 4; off <<= 1) {
        TGP_GU for (int i = 0; i < D; ++i) ga.gl[i] += __shfl_xor(ga.gl[i], off, 64);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lml += __shfl_xor(lml, off, 64);
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
        const double of = __shfl_xor(dist_f, off, 64), ob = __shfl_xor(dist_b, off, 64);
        dist_f = (of > dist_f) ? of : dist_f;
        dist_b = (ob > dist_b) ? ob : dist_b;
    }
    double* p = ka.part + (size_t)wave * (4 + tgp_sweep::group_adjoint_sde_sums(D));
    if (lane == 0) {
        p[0] = lml;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
        TGP_GU for (int i = 0; i < D; ++i) p[4 + i] = ga.gl[i];
        p[4 + D + 2 * D * D + DS + 2 * D] = ga.gh;
        p[4 + D + 2 * D * D + DS + 2 * D + 1] = ga.gR;
    }
    if (lane < D) {
        double* q = p + 4 + D;
        TGP_GU for (int i = 0; i < D; ++i) {
            q[i + D * j] = ga.gN1[i];
            q[D * D + i + D * j] = ga.gN2[i];
        }
        q += 2 * D * D;
        TGP_GU for (int i = 0; i < D; ++i)
            if (i <= j) q[j * (j + 1) / 2 + i] = ga.gPi[i];
        q += DS;
        q[j] = ga.ga;
        q += D;
        q[j] = ga.gH;
        q += D + 2;
        q[j] = gxm;
        q += D;
        TGP_GU for (int i = 0; i < D; ++i)
            if (i <= j) q[j * (j + 1) / 2 + i] = gxP[i];
    }
}

namespace {

template <int D> void launch_d(unsigned nwaves, hipStream_t stream, const GASArgs& ar) {
    const dim3 grid(nwaves), block(64);
    const int xs = (ar.gs.ka.st.R != nullptr ? 1 : 0) | (ar.gs.ka.st.hh != nullptr ? 2 : 0);
    switch (xs) {
        case 0: hipLaunchKernelGGL((k_sweep_group_adjoint_sde<D, 0>), grid, block, 0, stream, ar); break;
        case 1: hipLaunchKernelGGL((k_sweep_group_adjoint_sde<D, 1>), grid, block, 0, stream, ar); break;
        case 2: hipLaunchKernelGGL((k_sweep_group_adjoint_sde<D, 2>), grid, block, 0, stream, ar); break;
        default: hipLaunchKernelGGL((k_sweep_group_adjoint_sde<D, 3>), grid, block, 0, stream, ar); break;
    }
}

}  // namespace

void launch_adjoint_sde(int d, unsigned nwaves, hipStream_t stream, const GArgs& ka, const tgp_sweep::GroupSdeC& sc, double* gh_steps, double* gR_steps) {
    GASArgs ar;
    ar.gs.ka = ka;
    ar.gs.sc = sc;
    ar.gh_steps = gh_steps;
    ar.gR_steps = gR_steps;
    switch (d) {
        case 5: launch_d<5>(nwaves, stream, ar); break;
        case 6: launch_d<6>(nwaves, stream, ar); break;
        case 7: launch_d<7>(nwaves, stream, ar); break;
        default: launch_d<8>(nwaves, stream, ar); break;
    }
}

}  // namespace tgp_sweep_group
