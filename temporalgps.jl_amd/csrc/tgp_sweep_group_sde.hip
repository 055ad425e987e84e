// The group sweep on SDE-described models: k_sweep_group's algorithm and geometry (tgp_sweep_group.hip) with the transition
// of every step built from its gap, per group: A_t = diag(e) (I + tau N1 + tau^2 N2), e_i = exp(-lam_i tau) (tgp_sweep_body.hpp sde_A).  A_t is never
// written anywhere: N1 and N2 sit in LDS as two constant wave-wide broadcasts in A's place and a product with A_t is
// y_i = e_i (x_i + tau (N1 x)_i + tau^2 (N2 x)_i), over the band |i - k| <= 2 that the closed form's blocks fill (tgp_sweep_plan.hpp GroupSdeC).
// Q_t is never formed either: P_p = Pinf + A (P_f - Pinf) A', and where the RTS step needs A P_f itself, A P_f and A Pinf separately (predict_r).
// The series' first transition is no exp(F tau): the host predicts the prior through it and the kernel keeps that state at t == 0.
// A wave's LDS: N1 and N2 (2 x 512 B), the 8 groups' exchange tiles (8 x 82 doubles) and, in a posterior call, the filtering states of one checkpoint
// block per group: 6272 B (logpdf), 16 512 / 20 096 / 15 232 / 17 536 B at d = 5 / 6 / 7 / 8 (posterior).  gfx950 only.
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

// tgp_sweep_group.hip backward_run; the smoothing step t + 1 -> t takes the gap in front of step t + 1: the next lane's of the row, or behind a row's
// last step the first gap of the row (block, chunk) behind it -- the lane sweep's tau_next
template <int D, int XS, int B, bool EMIT>
__device__ __forceinline__ void backward_run_s(const GArgs& ka, const LaneS<D, XS>& ln, long long t0, int nrows, long long hi, bool fresh, GState<D>& xs, const double* ck,
                                               size_t ck_ld, double* sF, bool& ok) {
    constexpr int NS = LaneS<D, XS>::NS;
    RowS<XS> in, nx;
    load_row_s<XS>(ka, t0 + 8ll * (nrows - 1), ln.j, in);
    double tau_next = ka.st.tau[tgp_sweep::clamp_t(t0 + 8ll * nrows, ka.T)];
    for (int r = nrows - 1; r >= 0; --r) {
        const long long tb = t0 + 8ll * r;
        load_row_s<XS>(ka, tb - 8, ln.j, nx);      // the next row (row r - 1): in flight through this one
        double om = 0.0, ov = 0.0, rn = 0.0;
        if (EMIT) rn = ka.st.Rnew[ka.st.rnew_per_step ? tgp_sweep::clamp_t(tb + ln.j, ka.T) : 0];
#pragma nounroll
        for (int s = 8 / B - 1; s >= 0; --s) {
            const long long tsb = tb + s * B;
            if (tsb < hi) {
                // ---- the block's filtering states, forwards from its checkpoint
                GState<D> x;
                ln.load_packed(ck + (size_t)((tsb - t0) / B) * ck_ld, x);
                wave_sync();
#pragma nounroll
                for (int k = 0; k < B; ++k) {
                    ln.fstep(x, in, s * B + k, tsb + k, ka.T, (LmlAcc*)nullptr, ok);
                    ln.store_packed(sF + k * NS, x);
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
                        if (fresh && t == hi - 1) {
                            xs = xf;
                        } else {
                            const double tn = __shfl(in.tau, (q + 1) & 7, G);
                            StepA<D> sa;
                            ln.step_A(q == 7 ? tau_next : tn, sa);
                            ln.smooth_step(sa, xf, xs, ok);
                        }
                        if (EMIT) {
                            double mu, vr;
                            ln.emit(xs, (XS & 2) ? __shfl(in.hh, q, G) : ln.hh, mu, vr);
                            om = (ln.j == q) ? mu : om;
                            ov = (ln.j == q) ? vr : ov;
                        }
                    }
                }
            }
        }
        if (EMIT && tb + ln.j < hi) {
            ka.mean[tb + ln.j] = om;
            ka.var[tb + ln.j] = ov + rn;
        }
        tau_next = __shfl(in.tau, 0, G);
        in = nx;
    }
}

// k_sweep_group's frame (two forward passes, the hand-over checks, the backward warm-up and chunk, the wave's share).  The register counts are in
// profiles/sweep_group_sde_resources.txt.
template <int D, int XS, bool POST>
__global__ __launch_bounds__(64) void k_sweep_group_sde(const GSArgs by_value) {
    (void)by_value;
    const GSArgs& ar = *(const GSArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place: tgp_sweep.hip k_sweep)
    const GArgs& ka = ar.ka;
    constexpr int B = tgp_sweep::group_block(D), NS = LaneS<D, XS>::NS, NG = tgp_sweep::kGroupsPerWave;
    __shared__ __attribute__((aligned(16))) double sN[2 * G * G];
    __shared__ double tiles[NG * kTileLD];
    __shared__ double sF[POST ? NG * B * NS : 1];
    const int lane = threadIdx.x, g = lane / G;
    const long long wave = blockIdx.x;
    sN[lane] = ar.sc.N1[lane];
    sN[G * G + lane] = ar.sc.N2[lane];
    __syncthreads();

    LaneS<D, XS> ln;
    ln.j = lane % G;
    ln.act = ln.j < D;
    ln.tile = tiles + g * kTileLD;
    ln.sA = nullptr;
    ln.sN1 = sN;
    ln.sN2 = sN + G * G;
    const int j = ln.j;
    TGP_GU for (int i = 0; i < D; ++i) {
        ln.Gc[i] = ln.act ? ka.mc.gP[i + G * j] : 0.0;
        ln.lam[i] = ar.sc.lam[i];
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
    const bool runs = span.runs;
    const bool owned = span.owned;
    bool ok = true;

    GState<D> gen, x0;      // gen: (x0m, Pinf), where a warm-up starts from; x0: the state in front of update 0
    gen.m = ln.act ? ka.mc.gm[j] : 0.0;
    x0.m = ln.act ? ka.mc.x0m[j] : 0.0;
    TGP_GU for (int i = 0; i < D; ++i) {
        gen.P[i] = ln.Gc[i];
        x0.P[i] = ln.act ? ka.mc.x0P[i + G * j] : 0.0;
    }
    const size_t ck_ld = (size_t)NG * NS;
    double* ck = POST ? ka.ckpt + (size_t)wave * (size_t)(C / B) * ck_ld + (size_t)g * NS : nullptr;
    double* sFg = sF + (POST ? g * B * NS : 0);

    // ---- forwards: the warm-up over the last W steps of the chunk (its end state is the NEXT group's start state), then the chunk
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

    if (POST) {
        // ---- backwards, the warm-up over the chunk's first Wb steps (what the PREVIOUS group continues from), then the chunk
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // (the checkpoints are read back by other lanes of the group)
        const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
        GState<D> b1 = gen;
        backward_run_s<D, XS, B, false>(ka, ln, t0, ka.Wb / 8, runs ? te : t0, true, b1, ck, ck_ld, sFg, ok);
        GState<D> xs;
        xs.m = __shfl_down(b1.m, G, 64);
        TGP_GU for (int i = 0; i < D; ++i) xs.P[i] = __shfl_down(b1.P[i], G, 64);
        backward_run_s<D, XS, B, true>(ka, ln, t0, C / 8, owned ? t1 : t0, t1 == T, xs, ck, ck_ld, sFg, ok);
        const double db = ln.distance(ka.mc, xs, b1);
        const bool fin = ln.finite(xs) && ln.finite(b1);
        if (owned) {
            dist_b = db;
            finite = finite && fin;
        }
    }

    // ---- the wave's share: fixed-order sums over the groups (every lane of a group holds the same sums: lane 0 of each contributes)
    double lml = (owned && j == 0) ? acc.total() : 0.0;
    finite = finite && (::fabs(lml) < 1e300);
    unsigned bits = 0;
    if (owned && !(dist_f <= ka.mc.tol)) bits |= 1u;
    if (owned && POST && !(dist_b <= ka.mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lml += __shfl_xor(lml, off, 64);
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
        const double of = __shfl_xor(dist_f, off, 64), ob = __shfl_xor(dist_b, off, 64);
        dist_f = (of > dist_f) ? of : dist_f;
        dist_b = (ob > dist_b) ? ob : dist_b;
    }
    if (lane == 0) {
        double* p = ka.part + (size_t)wave * 4;
        p[0] = lml;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
    }
}

namespace {

template <int D, int XS> void launch_x(unsigned nwaves, hipStream_t stream, const GSArgs& ar, bool post) {
    if (post) hipLaunchKernelGGL((k_sweep_group_sde<D, XS, true>), dim3(nwaves), dim3(64), 0, stream, ar);
    else hipLaunchKernelGGL((k_sweep_group_sde<D, XS, false>), dim3(nwaves), dim3(64), 0, stream, ar);
}
template <int D> void launch_d(unsigned nwaves, hipStream_t stream, const GSArgs& ar, bool post) {
    const int xs = (ar.ka.st.R != nullptr ? 1 : 0) | (ar.ka.st.hh != nullptr ? 2 : 0);
    switch (xs) {
        case 0: launch_x<D, 0>(nwaves, stream, ar, post); break;
        case 1: launch_x<D, 1>(nwaves, stream, ar, post); break;
        case 2: launch_x<D, 2>(nwaves, stream, ar, post); break;
        default: launch_x<D, 3>(nwaves, stream, ar, post); break;
    }
}

}  // namespace

void launch_sde(int d, unsigned nwaves, hipStream_t stream, const GArgs& ka, const tgp_sweep::GroupSdeC& sc, bool post) {
    GSArgs ar;
    ar.ka = ka;
    ar.sc = sc;
    switch (d) {
        case 5: launch_d<5>(nwaves, stream, ar, post); break;
        case 6: launch_d<6>(nwaves, stream, ar, post); break;
        case 7: launch_d<7>(nwaves, stream, ar, post); break;
        default: launch_d<8>(nwaves, stream, ar, post); break;
    }
}

}  // namespace tgp_sweep_group
