// The group sweep: see tgp_sweep_group.hpp (what and why) and DESIGN 4.10 (geometry, LDS budget, register counts).  gfx950 only.
// One wave per workgroup; a wave's LDS: A (512 B), the 8 groups' exchange tiles (8 x 82 doubles) and, in a posterior call, the filtering states of
// one checkpoint block per group (8 B (d + d (d + 1) / 2) doubles: 13.5 KB at d = 6, B = 8; 11 KB at d = 8, B = 4) -- at most 19.6 KB, so that 8
// workgroups = two waves per SIMD stay resident in a CU's 160 KB.  An adjoint call (k_sweep_group_adjoint) has the posterior call's LDS: a block's slots hold
// the states in FRONT of its steps.
//
// The column layout and its building blocks are tgp_group.hpp's (GroupLane::predict, group_sum, gather) and tgp_group_smooth.hpp's (the 8-lane
// Cholesky solve); the recursions are tgp_sweep_body.hpp's update / smooth_step (a missing step: predict only; the RTS step in gain form).
// Lanes j >= d of a group hold zeros in every column they own, contribute exact zeros to every group sum and never write the tile rows >= d.
#include "tgp_sweep_group_dev.hpp"
#include "tgp_alloc.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace tgp_sweep_group {

// One forward run of a group: `nrows` rows of 8 steps from step ts on (a multiple of 8, possibly negative); the rows that start in [lo, hi) are
// processed, whole (steps behind the series' end are missing).  ck (null: none): the state in front of every block of B steps is kept, block
// (t - ck_t0) / B of the group's checkpoint array (stride ck_ld doubles).
template <int D, int XS, int B, bool KA>
__device__ __forceinline__ void forward_run(const GArgs& ka, const Lane<D, XS, KA>& ln, long long ts, int nrows, long long lo, long long hi, GState<D>& x, LmlAcc& acc,
                                            bool want_lml, double* ck, long long ck_t0, size_t ck_ld, bool& ok) {
    Row<XS> in, nx;
    load_row<XS>(ka, ts, ln.j, in);
    for (int r = 0; r < nrows; ++r) {
        const long long tb = ts + 8ll * r;
        load_row<XS>(ka, tb + 8, ln.j, nx);      // in flight while this row computes (behind the last row: clamped, unused)
        if (tb >= lo && tb < hi) {
            // (rolled in the posterior kernels: a step is hundreds of instructions, and eight copies of it only stretch the live ranges)
#pragma unroll(KA ? 8 : 1)
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

// One backward run of a group over the rows nrows - 1 .. 0 of its chunk (first step t0): the steps below hi are smoothed.  fresh: the run starts at
// step hi - 1 from that step's filtering state (the end of the series, or a warm-up); otherwise xs holds the smoothing state of step hi (the next
// group's first step).  On return xs is the smoothing state of step t0.  EMIT: mean / var of the steps are written, a 64-byte row per group.
// The filtering states of a block are recomputed from its checkpoint into LDS (sF: [step][NS] of this group).
template <int D, int XS, int B, bool EMIT, bool KA>
__device__ __forceinline__ void backward_run(const GArgs& ka, const Lane<D, XS, KA>& ln, long long t0, int nrows, long long hi, bool fresh, GState<D>& xs,
                                             const double* ck, size_t ck_ld, double* sF, bool& ok) {
    constexpr int NS = Lane<D, XS, KA>::NS;
    Row<XS> in, nx;
    load_row<XS>(ka, t0 + 8ll * (nrows - 1), ln.j, in);
    for (int r = nrows - 1; r >= 0; --r) {
        const long long tb = t0 + 8ll * r;
        load_row<XS>(ka, tb - 8, ln.j, nx);      // the next row (row r - 1): in flight through this one
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
                        GState<D> xf;
                        ln.load_packed(sF + k * NS, xf);
                        if (fresh && t == hi - 1) xs = xf;
                        else ln.smooth_step(xf, xs, ok);
                        if (EMIT) {
                            double mu, vr;
                            ln.emit(xs, (XS & 2) ? __shfl(in.hh, s * B + k, G) : ln.hh, mu, vr);
                            om = (ln.j == s * B + k) ? mu : om;
                            ov = (ln.j == s * B + k) ? vr : ov;
                        }
                    }
                }
            }
        }
        if (EMIT && tb + ln.j < hi) {
            ka.mean[tb + ln.j] = om;
            ka.var[tb + ln.j] = ov + rn;
        }
        in = nx;
    }
}

// (no register cap: under amdgpu_waves_per_eu(2) the posterior kernels spill from d = 6 on -- 28 to 560 bytes of scratch -- and a sequential
//  recursion pays for every spilled value in its dependent chain; the counts are in profiles/sweep_group_resources.txt)
template <int D, int XS, bool POST>
__global__ __launch_bounds__(64) void k_sweep_group(const GArgs by_value) {
    (void)by_value;
    const GArgs& ka = *(const GArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place: tgp_sweep.hip k_sweep)
    constexpr int B = tgp_sweep::group_block(D), NS = Lane<D, XS, !POST>::NS, NG = tgp_sweep::kGroupsPerWave;
    __shared__ __attribute__((aligned(16))) double sA[G * G];
    __shared__ double tiles[NG * kTileLD];
    __shared__ double sF[POST ? NG * B * NS : 1];
    const int lane = threadIdx.x, g = lane / G;
    const long long wave = blockIdx.x;
    sA[lane] = ka.mc.A[lane];
    __syncthreads();

    Lane<D, XS, !POST> ln;
    ln.j = lane % G;
    ln.act = ln.j < D;
    ln.tile = tiles + g * kTileLD;
    ln.sA = sA;
    const int j = ln.j;
    TGP_GU for (int i = 0; i < D; ++i) {
        ln.Qc[i] = ln.act ? ka.mc.Q[i + G * j] : 0.0;
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
    const long long t1r = (t1 + 7) & ~7ll;                 // the runs work in whole rows: the steps behind the series' end are missing ones
    const bool runs = span.runs;                           // group 0 only warms up for group 1
    const bool owned = span.owned;                         // (posterior calls) group 7 only warms up backwards for group 6
    bool ok = true;

    GState<D> gen, x0;
    gen.m = ln.act ? ka.mc.gm[j] : 0.0;
    x0.m = ln.act ? ka.mc.x0m[j] : 0.0;
    TGP_GU for (int i = 0; i < D; ++i) {
        gen.P[i] = ln.act ? ka.mc.gP[i + G * j] : 0.0;
        x0.P[i] = ln.act ? ka.mc.x0P[i + G * j] : 0.0;
    }
    const size_t ck_ld = (size_t)NG * NS;
    double* ck = POST ? ka.ckpt + (size_t)wave * (size_t)(C / B) * ck_ld + (size_t)g * NS : nullptr;
    double* sFg = sF + (POST ? g * B * NS : 0);

    // ---- forwards.  Pass 0: the last W steps of the chunk from the stationary prior (from x0 where they reach the series' first step); its end
    // state is the NEXT group's start state.  Pass 1: the chunk from the previous group's end state (checkpoints, log marginal likelihood).
    GState<D> x, e1;
    LmlAcc acc;
    {
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        forward_run<D, XS, B, !POST>(ka, ln, tw, ka.W / 8, tw > 0 ? tw : 0, t1r, x, acc, false, (double*)nullptr, 0, 0, ok);
        e1 = x;
        x.m = __shfl_up(e1.m, G, 64);
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] = __shfl_up(e1.P[i], G, 64);
        if (t0 == 0) x = x0;
        acc = LmlAcc();
        forward_run<D, XS, B, !POST>(ka, ln, t0, C / 8, t0, runs ? t1r : t0, x, acc, true, ck, t0, ck_ld, ok);
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
        // ---- backwards, the warm-up: the smoothing state of the chunk's first step as its first Wb steps give it from the filtering state behind
        // them (exact where they reach the series' last step) -- what the PREVIOUS group continues from
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");      // (the checkpoints are read back by other lanes of the group)
        const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
        GState<D> b1 = gen;
        backward_run<D, XS, B, false, !POST>(ka, ln, t0, ka.Wb / 8, runs ? te : t0, true, b1, ck, ck_ld, sFg, ok);
        // ---- backwards, the chunk: from the next group's smoothing state of ITS first step; mean and variance of every step
        GState<D> xs;
        xs.m = __shfl_down(b1.m, G, 64);
        TGP_GU for (int i = 0; i < D; ++i) xs.P[i] = __shfl_down(b1.P[i], G, 64);
        backward_run<D, XS, B, true, !POST>(ka, ln, t0, C / 8, owned ? t1 : t0, t1 == T, xs, ck, ck_ld, sFg, ok);
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

// ---- the adjoint gradient: k_sweep_adjoint's algorithm (tgp_sweep.hip) in k_sweep_group<POST>'s geometry ------------------
struct GAArgs {
    GArgs ka;              // (ka.Wb holds the adjoint's warm-up Wa; mean / var unused)
    double* gh_steps;      // [T] or null: d logpdf / d h_t, d logpdf / d R_t of every step
    double* gR_steps;
};
static_assert(sizeof(GAArgs) <= 4096, "the kernel's argument segment");

// One adjoint run of a group over the rows nrows - 1 .. 0 of its chunk (first step t0; backward_run's frame): the steps below hi are walked, from
// `ad` = the adjoint behind step hi - 1; on return `ad` is the adjoint in front of step t0.  The filtering states of a block are recomputed from its
// checkpoint into LDS (sF: [B][NS] of this group); step k reads the state in FRONT of it -- slot k holds the checkpoint for k = 0, step k - 1's
// state otherwise -- so the block's last state is not computed.  ACC: the block gradients are summed into *acc, and gh_t / gR_t of the walked
// steps are written where gh_steps / gR_steps are given, a 64-byte row per group.
template <int D, int XS, int B, bool ACC>
__device__ __forceinline__ void adjoint_run(const GArgs& ka, const Lane<D, XS, false>& ln, long long t0, int nrows, long long hi, GState<D>& ad, GAcc<D>* acc,
                                            double* gh_steps, double* gR_steps, const double* ck, size_t ck_ld, double* sF, bool& ok) {
    constexpr int NS = Lane<D, XS, false>::NS;
    Row<XS> in, nx;
    load_row<XS>(ka, t0 + 8ll * (nrows - 1), ln.j, in);
    for (int r = nrows - 1; r >= 0; --r) {
        const long long tb = t0 + 8ll * r;
        load_row<XS>(ka, tb - 8, ln.j, nx);      // the next row (row r - 1): in flight through this one
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
                        double gh_t, gR_t;
                        ln.template adjoint_step<ACC>(xf, y, Rt, ht, obs, ad, acc, gh_t, gR_t);
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

// part[wave]: [lml, bits, dist_f, dist_b | gA d*d | ga d | gQ packed | gH d | sum gh_t | sum gR_t | gx0m d | gx0P packed] -- k_sweep_adjoint's record
// (the symmetric blocks leave as the upper triangle of the lanes' columns).  The register counts are in profiles/sweep_group_adjoint_resources.txt.
template <int D, int XS>
__global__ __launch_bounds__(64) void k_sweep_group_adjoint(const GAArgs by_value) {
    (void)by_value;
    const GAArgs& ar = *(const GAArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place: tgp_sweep.hip k_sweep)
    const GArgs& ka = ar.ka;
    constexpr int B = tgp_sweep::group_block(D), NS = Lane<D, XS, false>::NS, DS = D * (D + 1) / 2, NG = tgp_sweep::kGroupsPerWave;
    __shared__ __attribute__((aligned(16))) double sA[G * G];
    __shared__ double tiles[NG * kTileLD];
    __shared__ double sF[NG * B * NS];
    const int lane = threadIdx.x, g = lane / G;
    const long long wave = blockIdx.x;
    sA[lane] = ka.mc.A[lane];
    __syncthreads();

    Lane<D, XS, false> ln;
    ln.j = lane % G;
    ln.act = ln.j < D;
    ln.tile = tiles + g * kTileLD;
    ln.sA = sA;
    const int j = ln.j;
    TGP_GU for (int i = 0; i < D; ++i) {
        ln.Qc[i] = ln.act ? ka.mc.Q[i + G * j] : 0.0;
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

    GState<D> gen, x0;
    gen.m = ln.act ? ka.mc.gm[j] : 0.0;
    x0.m = ln.act ? ka.mc.x0m[j] : 0.0;
    TGP_GU for (int i = 0; i < D; ++i) {
        gen.P[i] = ln.act ? ka.mc.gP[i + G * j] : 0.0;
        x0.P[i] = ln.act ? ka.mc.x0P[i + G * j] : 0.0;
    }
    const size_t ck_ld = (size_t)NG * NS;
    double* ck = ka.ckpt + (size_t)wave * (size_t)(C / B) * ck_ld + (size_t)g * NS;
    double* sFg = sF + g * B * NS;

    // ---- forwards: k_sweep_group<POST>'s two passes (warm-up, hand-over, the chunk with its checkpoints and the log marginal likelihood)
    GState<D> x, e1;
    LmlAcc acc;
    {
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        forward_run<D, XS, B, false>(ka, ln, tw, ka.W / 8, tw > 0 ? tw : 0, t1r, x, acc, false, (double*)nullptr, 0, 0, ok);
        e1 = x;
        x.m = __shfl_up(e1.m, G, 64);
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] = __shfl_up(e1.P[i], G, 64);
        if (t0 == 0) x = x0;
        acc = LmlAcc();
        forward_run<D, XS, B, false>(ka, ln, t0, C / 8, t0, runs ? t1r : t0, x, acc, true, ck, t0, ck_ld, ok);
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
        adjoint_run<D, XS, B, false>(ka, ln, t0, ka.Wb / 8, runs ? te : t0, b1, (GAcc<D>*)nullptr, (double*)nullptr, (double*)nullptr, ck, ck_ld, sFg, ok);
    }
    // ---- backwards, the chunk: from the next group's adjoint in front of ITS first step (zero behind the series' last step)
    GState<D> ad;
    ad.m = __shfl_down(b1.m, G, 64);
    TGP_GU for (int i = 0; i < D; ++i) ad.P[i] = __shfl_down(b1.P[i], G, 64);
    if (t1 == T) {
        ad.m = 0.0;
        TGP_GU for (int i = 0; i < D; ++i) ad.P[i] = 0.0;
    }
    GAcc<D> ga;
    ga.zero();
    adjoint_run<D, XS, B, true>(ka, ln, t0, C / 8, owned ? t1 : t0, ad, &ga, ar.gh_steps, ar.gR_steps, ck, ck_ld, sFg, ok);
    {
        const double db = ln.adjoint_distance(ka.mc, ad, b1);
        const bool fin = ln.finite(ad) && ln.finite(b1);
        if (owned) {
            dist_b = db;
            finite = finite && fin;
        }
    }

    // ---- the wave's share: the groups' sums added in a fixed order (lane j of every group holds column j), then lanes 0 .. d - 1 write their columns
    const bool first = owned && span.t0 == 0;      // the adjoint in front of step 0 is the gradient of the series' prior
    double gxm = first ? ad.m : 0.0, gxP[D];
    TGP_GU for (int i = 0; i < D; ++i) gxP[i] = first ? ad.P[i] : 0.0;
    {
        double s = ::fabs(ga.ga) + ::fabs(ga.gH) + ::fabs(ga.gh) + ::fabs(ga.gR);
        TGP_GU for (int i = 0; i < D; ++i) s += ::fabs(ga.gA[i]) + ::fabs(ga.gQ[i]);
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
            ga.gA[i] += __shfl_xor(ga.gA[i], off, 64);
            ga.gQ[i] += __shfl_xor(ga.gQ[i], off, 64);
            gxP[i] += __shfl_xor(gxP[i], off, 64);
        }
        ga.ga += __shfl_xor(ga.ga, off, 64);
        ga.gH += __shfl_xor(ga.gH, off, 64);
        ga.gh += __shfl_xor(ga.gh, off, 64);
        ga.gR += __shfl_xor(ga.gR, off, 64);
        gxm += __shfl_xor(gxm, off, 64);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lml += __shfl_xor(lml, off, 64);
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
        const double of = __shfl_xor(dist_f, off, 64), ob = __shfl_xor(dist_b, off, 64);
        dist_f = (of > dist_f) ? of : dist_f;
        dist_b = (ob > dist_b) ? ob : dist_b;
    }
    double* p = ka.part + (size_t)wave * (4 + tgp_sweep::group_adjoint_sums(D));
    if (lane == 0) {
        p[0] = lml;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
        p[4 + D * D + D + DS + D] = ga.gh;
        p[4 + D * D + D + DS + D + 1] = ga.gR;
    }
    if (lane < D) {
        double* q = p + 4;
        TGP_GU for (int i = 0; i < D; ++i) q[i + D * j] = ga.gA[i];
        q += D * D;
        q[j] = ga.ga;
        q += D;
        TGP_GU for (int i = 0; i < D; ++i)
            if (i <= j) q[j * (j + 1) / 2 + i] = ga.gQ[i];
        q += DS;
        q[j] = ga.gH;
        q += D + 2;
        q[j] = gxm;
        q += D;
        TGP_GU for (int i = 0; i < D; ++i)
            if (i <= j) q[j * (j + 1) / 2 + i] = gxP[i];
    }
}

// ---- a draw from the posterior: k_sweep_draw's walk (tgp_sweep.hip) in k_sweep_group<POST>'s geometry -----------------------
struct GDArgs {
    GArgs ka;               // (ka.Wb holds the draw's warm-up Wd; mean / var unused)
    const double* eps_t;    // [T][d]: row t drives the reverse-time transition out of step t (row 0 unused)
    const double* eps_e;    // [T]
    double eps_0[G];        // the start x_(T-1)
    double* y_out;          // [T]
};
static_assert(sizeof(GDArgs) <= 4096, "the kernel's argument segment");

// the draws of the transition out of step t, one per lane of the group (lane k < d holds eps_t[t][k])
template <int D> __device__ __forceinline__ double load_eps(const GDArgs& ar, long long t, int j) {
    return j < D ? ar.eps_t[(size_t)tgp_sweep::clamp_t(t, ar.ka.T) * D + j] : 0.0;
}

// One run of the walk by a group over the rows nrows - 1 .. 0 of its chunk (first step t0; backward_run's frame): the steps below hi are walked.
// start 0: x holds the sample of step hi (the next group's first step); 1: the run starts at step hi - 1 from that step's filtering mean (a warm-up);
// 2: from the true x_(T-1) = mf + chol(Pf + 1e-12 I).U' eps_0 (step hi - 1 is the series' last).  On return x is the sample of step t0.
// EMIT: y*_t = H x_t + h_t + sqrt(Rnew_t) eps_e[t] of the steps is written, a 64-byte row per group.  The draws of a step are asked for one step ahead
// (a row of lanes, handed out by shuffle); the filtering states of a block are recomputed from its checkpoint into LDS (sF: [step][NS] of this group).
template <int D, int XS, int B, bool EMIT>
__device__ __forceinline__ void draw_run(const GDArgs& ar, const Lane<D, XS, false>& ln, long long t0, int nrows, long long hi, int start, double& x,
                                         const double* ck, size_t ck_ld, double* sF, bool& ok) {
    constexpr int NS = Lane<D, XS, false>::NS;
    const GArgs& ka = ar.ka;
    Row<XS> in, nx;
    load_row<XS>(ka, t0 + 8ll * (nrows - 1), ln.j, in);
    double en = load_eps<D>(ar, hi, ln.j);      // what step hi - 1 consumes (unused where the run starts there)
    for (int r = nrows - 1; r >= 0; --r) {
        const long long tb = t0 + 8ll * r;
        load_row<XS>(ka, tb - 8, ln.j, nx);      // the next row (row r - 1): in flight through this one
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
                        GState<D> xf;
                        ln.load_packed(sF + k * NS, xf);
                        const double ec = en;
                        en = load_eps<D>(ar, t, ln.j);      // step t - 1's draws: in flight through this step
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
                            ln.draw_step(xf, x, e, ok);
                        }
                        if (EMIT) {
                            const double hx = group_sum(ln.Hj * x) + ((XS & 2) ? __shfl(in.hh, s * B + k, G) : ln.hh);
                            oy = (ln.j == s * B + k) ? hx : oy;
                        }
                    }
                }
            }
        }
        if (EMIT && tb + ln.j < hi) ar.y_out[tb + ln.j] = fma(::sqrt(rn), ee, oy);
        in = nx;
    }
}

// part[wave]: [0, bits, dist_f, dist_d].  The register counts are in profiles/sweep_group_draw_resources.txt.
template <int D, int XS>
__global__ __launch_bounds__(64) void k_sweep_group_draw(const GDArgs by_value) {
    (void)by_value;
    const GDArgs& ar = *(const GDArgs*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place: tgp_sweep.hip k_sweep)
    const GArgs& ka = ar.ka;
    constexpr int B = tgp_sweep::group_block(D), NS = Lane<D, XS, false>::NS, NG = tgp_sweep::kGroupsPerWave;
    __shared__ __attribute__((aligned(16))) double sA[G * G];
    __shared__ double tiles[NG * kTileLD];
    __shared__ double sF[NG * B * NS];
    const int lane = threadIdx.x, g = lane / G;
    const long long wave = blockIdx.x;
    sA[lane] = ka.mc.A[lane];
    __syncthreads();

    Lane<D, XS, false> ln;
    ln.j = lane % G;
    ln.act = ln.j < D;
    ln.tile = tiles + g * kTileLD;
    ln.sA = sA;
    const int j = ln.j;
    TGP_GU for (int i = 0; i < D; ++i) {
        ln.Qc[i] = ln.act ? ka.mc.Q[i + G * j] : 0.0;
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

    GState<D> gen, x0;
    gen.m = ln.act ? ka.mc.gm[j] : 0.0;
    x0.m = ln.act ? ka.mc.x0m[j] : 0.0;
    TGP_GU for (int i = 0; i < D; ++i) {
        gen.P[i] = ln.act ? ka.mc.gP[i + G * j] : 0.0;
        x0.P[i] = ln.act ? ka.mc.x0P[i + G * j] : 0.0;
    }
    const size_t ck_ld = (size_t)NG * NS;
    double* ck = ka.ckpt + (size_t)wave * (size_t)(C / B) * ck_ld + (size_t)g * NS;
    double* sFg = sF + g * B * NS;

    // ---- forwards: k_sweep_group<POST>'s two passes (warm-up, hand-over, the chunk with its checkpoints); no log marginal likelihood
    GState<D> x, e1;
    {
        LmlAcc acc;
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        forward_run<D, XS, B, false>(ka, ln, tw, ka.W / 8, tw > 0 ? tw : 0, t1r, x, acc, false, (double*)nullptr, 0, 0, ok);
        e1 = x;
        x.m = __shfl_up(e1.m, G, 64);
        TGP_GU for (int i = 0; i < D; ++i) x.P[i] = __shfl_up(e1.P[i], G, 64);
        if (t0 == 0) x = x0;
        forward_run<D, XS, B, false>(ka, ln, t0, C / 8, t0, runs ? t1r : t0, x, acc, false, ck, t0, ck_ld, ok);
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
        draw_run<D, XS, B, false>(ar, ln, t0, ka.Wb / 8, runs ? te : t0, te == T ? 2 : 1, b1, ck, ck_ld, sFg, ok);
    }
    // ---- backwards, the chunk: from the next group's sample of ITS first step; y* of every step
    double xs = __shfl_down(b1, G, 64);
    draw_run<D, XS, B, true>(ar, ln, t0, C / 8, owned ? t1 : t0, t1 == T ? 2 : 0, xs, ck, ck_ld, sFg, ok);
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

// ------------------------------------------------------------------------------------------------------------------------ host side
struct Engine {
    tgp_sweep::GroupPlan p;
    tgp_sweep::Forced forced;
    double* part = nullptr;      // pinned: the waves' shares
    size_t part_cap = 0;
    int part_stride = 4;         // doubles per wave in `part`: 4, and the gradient's sums behind them in an adjoint call
    void* ckpt = nullptr;
    size_t ckpt_cap = 0;
};

Engine* create() { return new Engine(); }
void destroy(Engine* e) {
    if (!e) return;
    if (e->part) (void)tgp_alloc::host_free(e->part);
    if (e->ckpt) (void)tgp_alloc::dev_free(e->ckpt);
    delete e;
}
void force_geometry(Engine* e, int C, int W, int Wb) {
    e->forced.C = C;
    e->forced.W = W;
    e->forced.Wb = Wb;
}
void geometry(const Engine* e, int* C, int* W, int* Wb, int64_t* nwaves) {
    if (C) *C = e->p.C;
    if (W) *W = e->p.W;
    if (Wb) *Wb = e->p.Wb;
    if (nwaves) *nwaves = e->p.nwaves;
}
bool plan(Engine* e, const tgp_sweep::ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, bool post, std::string* why, bool adjoint, bool draw) {
    return tgp_sweep::plan_group(&e->p, e->forced, m, T, w_hint, wb_hint, num_cu, post || adjoint || draw, why, adjoint, draw);
}
const char* kernel_name(bool post, bool sde) {
    if (sde) return post ? "k_sweep_group<sde,posterior>" : "k_sweep_group<sde,logpdf>";
    return post ? "k_sweep_group<lti,posterior>" : "k_sweep_group<lti,logpdf>";
}
const char* adjoint_kernel_name() { return "k_sweep_group_adjoint<lti>"; }
const char* draw_kernel_name() { return "k_sweep_group_draw<lti>"; }

namespace {

template <int D, int XS> void launch_x(const Engine* e, hipStream_t stream, const GArgs& ka, bool post) {
    if (post) hipLaunchKernelGGL((k_sweep_group<D, XS, true>), dim3((unsigned)e->p.nwaves), dim3(64), 0, stream, ka);
    else hipLaunchKernelGGL((k_sweep_group<D, XS, false>), dim3((unsigned)e->p.nwaves), dim3(64), 0, stream, ka);
}
template <int D> void launch_d(const Engine* e, hipStream_t stream, const GArgs& ka, bool post) {
    const int xs = (ka.st.R != nullptr ? 1 : 0) | (ka.st.hh != nullptr ? 2 : 0);
    switch (xs) {
        case 0: launch_x<D, 0>(e, stream, ka, post); break;
        case 1: launch_x<D, 1>(e, stream, ka, post); break;
        case 2: launch_x<D, 2>(e, stream, ka, post); break;
        default: launch_x<D, 3>(e, stream, ka, post); break;
    }
}
template <int D> void launch_adjoint_d(const Engine* e, hipStream_t stream, const GAArgs& ar) {
    const dim3 grid((unsigned)e->p.nwaves), block(64);
    const int xs = (ar.ka.st.R != nullptr ? 1 : 0) | (ar.ka.st.hh != nullptr ? 2 : 0);
    switch (xs) {
        case 0: hipLaunchKernelGGL((k_sweep_group_adjoint<D, 0>), grid, block, 0, stream, ar); break;
        case 1: hipLaunchKernelGGL((k_sweep_group_adjoint<D, 1>), grid, block, 0, stream, ar); break;
        case 2: hipLaunchKernelGGL((k_sweep_group_adjoint<D, 2>), grid, block, 0, stream, ar); break;
        default: hipLaunchKernelGGL((k_sweep_group_adjoint<D, 3>), grid, block, 0, stream, ar); break;
    }
}

template <int D> void launch_draw_d(const Engine* e, hipStream_t stream, const GDArgs& ar) {
    const dim3 grid((unsigned)e->p.nwaves), block(64);
    const int xs = (ar.ka.st.R != nullptr ? 1 : 0) | (ar.ka.st.hh != nullptr ? 2 : 0);
    switch (xs) {
        case 0: hipLaunchKernelGGL((k_sweep_group_draw<D, 0>), grid, block, 0, stream, ar); break;
        case 1: hipLaunchKernelGGL((k_sweep_group_draw<D, 1>), grid, block, 0, stream, ar); break;
        case 2: hipLaunchKernelGGL((k_sweep_group_draw<D, 2>), grid, block, 0, stream, ar); break;
        default: hipLaunchKernelGGL((k_sweep_group_draw<D, 3>), grid, block, 0, stream, ar); break;
    }
}

}  // namespace

int enqueue(Engine* e, hipStream_t stream, const tgp_sweep::Call& c, const char** kname, std::string* err) {
    auto fail = [&](const char* what, hipError_t rc) {
        if (err) *err = std::string(what) + ": " + hipGetErrorString(rc);
        return 1;
    };
    const tgp_sweep::GroupPlan& p = e->p;
    const bool post = c.mean != nullptr;
    if (c.adjoint ? (post || !p.adjoint) : p.adjoint) {
        if (err) *err = "k_sweep_group_adjoint: the call does not match its plan (no other output in an adjoint call)";
        return 1;
    }
    const bool draw = c.y_out != nullptr;
    if (draw ? (post || c.adjoint || !p.draw || c.eps_t == nullptr || c.eps_e == nullptr || c.Rnew == nullptr) : p.draw) {
        if (err) *err = "k_sweep_group_draw: the call does not match its plan (no other output in a draw call)";
        return 1;
    }
    if ((post || c.adjoint || draw) != p.post || c.T != p.T || (post && (c.var == nullptr || c.Rnew == nullptr)) || (p.sde && c.tau == nullptr)) {
        if (err) *err = "k_sweep_group: the call does not match its plan";
        return 1;
    }
    e->part_stride = c.adjoint ? 4 + tgp_sweep::group_adjoint_sums(p.d) : 4;
    const size_t need_part = (size_t)p.nwaves * e->part_stride * sizeof(double);
    if (need_part > e->part_cap) {
        if (e->part) (void)tgp_alloc::host_free(e->part);
        e->part = nullptr;
        e->part_cap = 0;
        const size_t cap = std::max<size_t>(need_part, 1 << 16);
        hipError_t rc = tgp_alloc::host_malloc((void**)&e->part, cap, hipHostMallocDefault);
        if (rc != hipSuccess) return fail("hipHostMalloc", rc);
        e->part_cap = cap;
    }
    if (p.post) {      // (the adjoint keeps the posterior call's checkpoints)
        const int NS = p.d + p.d * (p.d + 1) / 2;
        const size_t need = (size_t)p.nwaves * (size_t)(p.C / p.B) * tgp_sweep::kGroupsPerWave * NS * sizeof(double);
        if (need > e->ckpt_cap) {
            if (e->ckpt) (void)tgp_alloc::dev_free(e->ckpt);
            e->ckpt = nullptr;
            e->ckpt_cap = 0;
            hipError_t rc = tgp_alloc::dev_malloc(&e->ckpt, need);
            if (rc != hipSuccess) return fail("hipMalloc", rc);
            e->ckpt_cap = need;
        }
    }
    GArgs ka;
    ka.mc = p.mc;
    ka.st.y = c.y;
    ka.st.mask = c.mask;
    ka.st.R = c.R;
    ka.st.hh = c.hh;
    ka.st.tau = nullptr;
    ka.st.Rnew = c.Rnew;
    ka.st.rnew_per_step = c.rnew_per_step;
    ka.T = p.T;
    ka.C = p.C;
    ka.W = p.W;
    ka.Wb = p.Wb;
    ka.owned = p.owned;
    ka.nchunks = p.nchunks;
    ka.mean = c.mean;
    ka.var = c.var;
    ka.ckpt = static_cast<double*>(e->ckpt);
    ka.part = e->part;
    if (c.adjoint) {
        GAArgs ar;
        ar.ka = ka;      // (ka.Wb: the plan's backward slot carries the adjoint's warm-up)
        ar.gh_steps = c.gh_steps;
        ar.gR_steps = c.gR_steps;
        if (kname) *kname = adjoint_kernel_name();
        switch (p.d) {
            case 5: launch_adjoint_d<5>(e, stream, ar); break;
            case 6: launch_adjoint_d<6>(e, stream, ar); break;
            case 7: launch_adjoint_d<7>(e, stream, ar); break;
            default: launch_adjoint_d<8>(e, stream, ar); break;
        }
        hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return fail("k_sweep_group_adjoint launch", rc);
        return 0;
    }
    if (draw) {
        GDArgs ar;
        ar.ka = ka;      // (ka.Wb: the plan's backward slot carries the draw's warm-up)
        ar.eps_t = c.eps_t;
        ar.eps_e = c.eps_e;
        for (int k = 0; k < G; ++k) ar.eps_0[k] = k < p.d ? c.eps_0[k] : 0.0;
        ar.y_out = c.y_out;
        if (kname) *kname = draw_kernel_name();
        switch (p.d) {
            case 5: launch_draw_d<5>(e, stream, ar); break;
            case 6: launch_draw_d<6>(e, stream, ar); break;
            case 7: launch_draw_d<7>(e, stream, ar); break;
            default: launch_draw_d<8>(e, stream, ar); break;
        }
        hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return fail("k_sweep_group_draw launch", rc);
        return 0;
    }
    if (kname) *kname = kernel_name(post, p.sde);
    if (p.sde) {      // an SDE-described model: the transitions from the gaps (tgp_sweep_group_sde.hip)
        ka.st.tau = c.tau;
        launch_sde(p.d, (unsigned)p.nwaves, stream, ka, p.sc, post);
        hipError_t rc = hipGetLastError();
        if (rc != hipSuccess) return fail("k_sweep_group_sde launch", rc);
        return 0;
    }
    switch (p.d) {
        case 5: launch_d<5>(e, stream, ka, post); break;
        case 6: launch_d<6>(e, stream, ka, post); break;
        case 7: launch_d<7>(e, stream, ka, post); break;
        default: launch_d<8>(e, stream, ka, post); break;
    }
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return fail("k_sweep_group launch", rc);
    return 0;
}

double finish(Engine* e, int* status, int* w, int* wb, double* dist_f, double* dist_b) {
    double lml = 0.0, df = 0.0, db = 0.0;
    unsigned bits = 0;
    for (int64_t i = 0; i < e->p.nwaves; ++i) {      // fixed order: the same sum for the same geometry
        const double* q = e->part + (size_t)i * e->part_stride;
        lml += q[0];
        bits |= (unsigned)q[1];
        df = std::max(df, q[2]);
        db = std::max(db, q[3]);
    }
    if (status) *status = (int)bits;
    if (w) *w = e->p.W;
    if (wb) *wb = e->p.Wb;
    if (dist_f) *dist_f = df;
    if (dist_b) *dist_b = db;
    return lml;
}

void adjoint_blocks(const Engine* e, const tgp_sweep::AdjointOut& out) {
    tgp_sweep::adjoint_blocks_from_parts(e->part, e->p.nwaves, e->part_stride, e->p.d, out);
}

}  // namespace tgp_sweep_group
