// The sweep engine: see tgp_sweep.hpp (what and why) and tgp_sweep_body.hpp (the per-lane arithmetic, shared with tests/hostsim).
// gfx950 only.  One wave per workgroup, one wave per SIMD (the kernel is bound by its fp64 instruction stream, not by memory: every
// lane carries the full covariance recursion of its chunk), 4 workgroups per CU by their LDS (the filtering states of a block).
#include "tgp_sweep.hpp"
#include "tgp_alloc.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tgp_sweep_body.hpp"

namespace tgp_sweep {

__device__ __forceinline__ double shfl_up1(double v) { return __shfl_up(v, 1, 64); }
__device__ __forceinline__ double shfl_dn1(double v) { return __shfl_down(v, 1, 64); }

template <int D> __device__ __forceinline__ bool state_finite(const State<D>& x) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < D; ++k) s += ::fabs(x.m[k]);
#pragma unroll
    for (int k = 0; k < SD<D>::DS; ++k) s += ::fabs(x.P[k]);
    return s < 1e300;      // (false for NaN as well)
}

template <int D, bool SDE, int XS, bool POST>
__global__ __launch_bounds__(64, 1) void k_sweep(const KArgs<D> by_value) {
    (void)by_value;
    const KArgs<D>& ka = *(const KArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place, scalar loads: tgp_modal.hip k_steady_one)
    constexpr int B = Geo<D>::B, NS = SD<D>::NS, DS = SD<D>::DS;
    constexpr int kStates = B * NS * 64, kTiles = 2 * 64 * (B + 1);      // the block's filtering states; later in a block, its two output tiles
    __shared__ double sF[POST ? (kStates > kTiles ? kStates : kTiles) : 64];
    const int lane = threadIdx.x;
    const long long wave = blockIdx.x;
    const long long T = ka.T;
    const int C = ka.C;
    const long long c = wave * kOwned + lane - 1;
    const bool active = c >= 0 && c < ka.nchunks;
    const long long t0 = active ? c * C : 0;
    long long t1 = active ? t0 + C : 0;
    t1 = t1 < T ? t1 : (active ? T : 0);
    const long long t1r = (t1 + 7) & ~7ll;                    // the runs work in whole blocks: the steps behind the series' end are missing ones
    const bool runs = active && lane >= 1;                    // lane 0 only warms up for lane 1
    const bool owned = runs && lane <= kOwned;                // lane 63 only warms up (backwards) for lane 62
    bool ok = true;

    ModelR<D, SDE> mr;
    mr.init(ka.mc);
    State<D> gen, x0;
    set_state<D>(gen, ka.mc.gm, ka.mc.gP);
    set_state<D>(x0, ka.mc.x0m, ka.mc.x0P);
    double* ck = POST ? ka.ckpt + (size_t)wave * (size_t)(C / B) * NS * 64 : nullptr;

    // ---- forwards.  Pass 0: the last W steps of the chunk from the stationary prior (from x0 where they reach the series' first step); its
    // end state is the NEXT lane's start state.  Pass 1: the chunk from the previous lane's end state (checkpoints, log marginal likelihood).
    State<D> x, e1;
    LmlAcc acc;
    // (POST) the smoothing state of the chunk's first step as its first Wb steps give it -- what the PREVIOUS lane continues from -- is composed
    // during the forward run (RevAcc): from the filtering state behind those steps (the smoothing state where they reach the series' last step)
    const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
    RevAcc<D> rev;
    rev.reset();
    State<D> b1 = gen;
    {
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        // segment 0: the warm-up; 1: (POST) the chunk's first Wb steps, with the reverse-time composition; 2: the rest of the chunk
        const int nwin = POST ? ka.Wb / B : 0;
        for (int seg = 0; seg < 3; ++seg) {
            if (seg == 1) {
                if constexpr (POST) forward_run<D, SDE, XS, B, true>(ka, mr, t0, nwin, t0, runs ? t1r : t0, x, acc, true, ck, lane, ok, &rev, t0, te, &b1);
            } else {      // (ONE call site for both plain runs: the loop body exists once)
                const bool warm = seg == 0;
                const long long ts = warm ? tw : t0 + (long long)nwin * B;
                forward_run<D, SDE, XS, B>(ka, mr, ts, warm ? ka.W / B : C / B - nwin, warm ? (tw > 0 ? tw : 0) : t0, warm ? t1r : (runs ? t1r : t0), x, acc, !warm,
                                           (POST && !warm) ? ck + (size_t)nwin * NS * 64 : (double*)nullptr, lane, ok);
                if (warm) {
                    e1 = x;
#pragma unroll
                    for (int k = 0; k < D; ++k) x.m[k] = shfl_up1(e1.m[k]);
#pragma unroll
                    for (int k = 0; k < DS; ++k) x.P[k] = shfl_up1(e1.P[k]);
                    if (t0 == 0) x = x0;
                    acc = LmlAcc();
                }
            }
        }
    }
    double dist_f = 0.0, dist_b = 0.0;
    bool finite = true;
    if (owned) {
        dist_f = state_distance<D>(ka.mc, x, e1);
        finite = state_finite<D>(x) && state_finite<D>(e1);
    }

    if (POST) {
        // ---- backwards: the chunk from the next lane's smoothing state of ITS first step; mean and variance of every step.
        State<D> xs;
#pragma unroll
        for (int k = 0; k < D; ++k) xs.m[k] = shfl_dn1(b1.m[k]);
#pragma unroll
        for (int k = 0; k < DS; ++k) xs.P[k] = shfl_dn1(b1.P[k]);
        backward_run<D, SDE, XS, B>(ka, mr, t0, C / B, owned ? t1 : t0, t1 == T, xs, true, ck, sF, lane, ok);
        if (owned) {
            dist_b = state_distance<D>(ka.mc, xs, b1);
            finite = finite && state_finite<D>(xs) && state_finite<D>(b1);
        }
    }

    // ---- the wave's share: fixed-order sums over the lanes
    double lml = owned ? acc.total() : 0.0;
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

// The posterior draw (tgp_sweep.hpp): k_sweep<POST>'s forward half -- warm-up, hand-over, checkpoints, dist_f -- with the walk over a
// chunk's first Wd steps composed on the way (DrawAcc; ka.Wb holds Wd), then the walk over the chunk from the next lane's sample state of ITS
// first step.  The check of the second hand-over compares sample states.
template <int D> struct DArgs {
    KArgs<D> ka;
    DrawArgs da;
};

template <int D, bool SDE, int XS>
__global__ __launch_bounds__(64, 1) void k_sweep_draw(const DArgs<D> by_value) {
    (void)by_value;
    const DArgs<D>& ar = *(const DArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();
    const KArgs<D>& ka = ar.ka;
    const DrawArgs& da = ar.da;
    constexpr int B = Geo<D>::B, NS = SD<D>::NS, DS = SD<D>::DS;
    __shared__ double sF[B * NS * 64];      // the block's filtering states; later in a block, its output tile (64 (B + 1) doubles)
    const int lane = threadIdx.x;
    const long long wave = blockIdx.x;
    const long long T = ka.T;
    const int C = ka.C;
    const long long c = wave * kOwned + lane - 1;
    const bool active = c >= 0 && c < ka.nchunks;
    const long long t0 = active ? c * C : 0;
    long long t1 = active ? t0 + C : 0;
    t1 = t1 < T ? t1 : (active ? T : 0);
    const long long t1r = (t1 + 7) & ~7ll;
    const bool runs = active && lane >= 1;
    const bool owned = runs && lane <= kOwned;
    bool ok = true;

    ModelR<D, SDE> mr;
    mr.init(ka.mc);
    State<D> gen, x0;
    set_state<D>(gen, ka.mc.gm, ka.mc.gP);
    set_state<D>(x0, ka.mc.x0m, ka.mc.x0P);
    double* ck = ka.ckpt + (size_t)wave * (size_t)(C / B) * NS * 64;

    State<D> x, e1;
    LmlAcc acc;
    const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
    DrawAcc<D> dr;
    dr.reset();
    double b1[D];
#pragma unroll
    for (int k = 0; k < D; ++k) b1[k] = gen.m[k];
    {
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        // segment 0: the warm-up; 1: the chunk's first Wd steps, with the walk composed; 2: the rest of the chunk
        const int nwin = ka.Wb / B;
        for (int seg = 0; seg < 3; ++seg) {
            if (seg == 1) {
                forward_run_draw<D, SDE, XS, B>(ka, da, mr, t0, nwin, t0, runs ? t1r : t0, x, ck, lane, ok, dr, t0, te, b1);
            } else {
                const bool warm = seg == 0;
                const long long ts = warm ? tw : t0 + (long long)nwin * B;
                forward_run<D, SDE, XS, B>(ka, mr, ts, warm ? ka.W / B : C / B - nwin, warm ? (tw > 0 ? tw : 0) : t0, warm ? t1r : (runs ? t1r : t0), x, acc, false,
                                           warm ? (double*)nullptr : ck + (size_t)nwin * NS * 64, lane, ok);
                if (warm) {
                    e1 = x;
#pragma unroll
                    for (int k = 0; k < D; ++k) x.m[k] = shfl_up1(e1.m[k]);
#pragma unroll
                    for (int k = 0; k < DS; ++k) x.P[k] = shfl_up1(e1.P[k]);
                    if (t0 == 0) x = x0;
                }
            }
        }
    }
    double dist_f = 0.0, dist_b = 0.0;
    bool finite = true;
    if (owned) {
        dist_f = state_distance<D>(ka.mc, x, e1);
        finite = state_finite<D>(x) && state_finite<D>(e1);
    }

    // ---- backwards: the chunk from the next lane's sample state of ITS first step; the emission of every step
    double xw[D];
#pragma unroll
    for (int k = 0; k < D; ++k) xw[k] = shfl_dn1(b1[k]);
    backward_run_draw<D, SDE, XS, B>(ka, da, mr, t0, C / B, owned ? t1 : t0, t1 == T, xw, ck, sF, lane, ok);
    if (owned) {
        dist_b = draw_distance<D>(ka.mc, xw, b1);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s += ::fabs(xw[k]) + ::fabs(b1[k]);
        finite = finite && (s < 1e300);
    }

    unsigned bits = 0;
    if (owned && !(dist_f <= ka.mc.tol)) bits |= 1u;
    if (owned && !(dist_b <= ka.mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
        const double of = __shfl_xor(dist_f, off, 64), ob = __shfl_xor(dist_b, off, 64);
        dist_f = (of > dist_f) ? of : dist_f;
        dist_b = (ob > dist_b) ? ob : dist_b;
    }
    if (lane == 0) {
        double* p = ka.part + (size_t)wave * 4;
        p[0] = 0.0;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
    }
}

// The adjoint gradient (tgp_sweep.hpp), LTI form: k_sweep<POST>'s forward half without the composed window -- warm-up, hand-over, checkpoints,
// the log marginal likelihood, dist_f -- then the adjoint of the recursion backwards: first over the chunk's first Wa steps from a zero adjoint (ka.Wb holds
// Wa; the result is what the PREVIOUS lane continues from), then over the chunk from the next lane's adjoint in front of ITS first step, summing the
// block gradients.  The check of the second hand-over compares adjoints.  part[wave]: [lml, bits, dist_f, dist_b | gA d*d | ga d | gQ packed | gH d |
// sum gh_t | sum gR_t | gx0m d | gx0P packed].
template <int D> struct AArgs {
    KArgs<D> ka;
    double* gh_steps;      // [T] or null
    double* gR_steps;
};
template <int D> struct AdjParts {
    static constexpr int NG = AdjAcc<D>::N + SD<D>::NS, STRIDE = 4 + NG;
};

template <int D, int XS>
__global__ __launch_bounds__(64, 1) void k_sweep_adjoint(const AArgs<D> by_value) {
    (void)by_value;
    const AArgs<D>& ar = *(const AArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();
    const KArgs<D>& ka = ar.ka;
    constexpr int B = Geo<D>::B, NS = SD<D>::NS, DS = SD<D>::DS;
    __shared__ double sF[B * NS * 64];      // the block's filtering states
    const int lane = threadIdx.x;
    const long long wave = blockIdx.x;
    const long long T = ka.T;
    const int C = ka.C;
    const long long c = wave * kOwned + lane - 1;
    const bool active = c >= 0 && c < ka.nchunks;
    const long long t0 = active ? c * C : 0;
    long long t1 = active ? t0 + C : 0;
    t1 = t1 < T ? t1 : (active ? T : 0);
    const long long t1r = (t1 + 7) & ~7ll;
    const bool runs = active && lane >= 1;
    const bool owned = runs && lane <= kOwned;
    bool ok = true;

    ModelR<D, false> mr;
    mr.init(ka.mc);
    State<D> gen, x0;
    set_state<D>(gen, ka.mc.gm, ka.mc.gP);
    set_state<D>(x0, ka.mc.x0m, ka.mc.x0P);
    double* ck = ka.ckpt + (size_t)wave * (size_t)(C / B) * NS * 64;

    // ---- forwards: the warm-up over the chunk's last W steps, the shift, the chunk with its checkpoints
    State<D> x, e1;
    LmlAcc acc;
    {
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        for (int seg = 0; seg < 2; ++seg) {      // (ONE call site for both runs: the loop body exists once)
            const bool warm = seg == 0;
            forward_run<D, false, XS, B>(ka, mr, warm ? tw : t0, warm ? ka.W / B : C / B, warm ? (tw > 0 ? tw : 0) : t0, warm ? t1r : (runs ? t1r : t0), x, acc, !warm,
                                         warm ? (double*)nullptr : ck, lane, ok);
            if (warm) {
                e1 = x;
#pragma unroll
                for (int k = 0; k < D; ++k) x.m[k] = shfl_up1(e1.m[k]);
#pragma unroll
                for (int k = 0; k < DS; ++k) x.P[k] = shfl_up1(e1.P[k]);
                if (t0 == 0) x = x0;
                acc = LmlAcc();
            }
        }
    }
    double dist_f = 0.0, dist_b = 0.0;
    bool finite = true;
    if (owned) {
        dist_f = state_distance<D>(ka.mc, x, e1);
        finite = state_finite<D>(x) && state_finite<D>(e1);
    }

    // ---- backwards, the warm-up: the adjoint in front of the chunk's first step as its first Wa steps give it from zero (exact where they reach the
    // series' last step)
    Adj<D> b1;
    b1.zero();
    {
        const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
        adjoint_run<D, XS, B, false>(ka, mr, t0, ka.Wb / B, runs ? te : t0, b1, (AdjAcc<D>*)nullptr, (double*)nullptr, (double*)nullptr, ck, sF, lane, ok);
    }
    // ---- backwards, the chunk: from the next lane's adjoint in front of ITS first step (zero behind the series' last step)
    Adj<D> ad;
#pragma unroll
    for (int k = 0; k < D; ++k) ad.l[k] = shfl_dn1(b1.l[k]);
#pragma unroll
    for (int k = 0; k < DS; ++k) ad.L[k] = shfl_dn1(b1.L[k]);
    if (t1 == T) ad.zero();
    AdjAcc<D> ga;
    ga.zero();
    adjoint_run<D, XS, B, true>(ka, mr, t0, C / B, owned ? t1 : t0, ad, &ga, ar.gh_steps, ar.gR_steps, ck, sF, lane, ok);

    // ---- the wave's share: fixed-order sums over the lanes
    constexpr int NG = AdjParts<D>::NG;
    double g[NG];
    {
        int n = 0;
#pragma unroll
        for (int k = 0; k < D * D; ++k) g[n++] = ga.gA[k];
#pragma unroll
        for (int k = 0; k < D; ++k) g[n++] = ga.ga[k];
#pragma unroll
        for (int k = 0; k < DS; ++k) g[n++] = ga.gQ[k];
#pragma unroll
        for (int k = 0; k < D; ++k) g[n++] = ga.gH[k];
        g[n++] = ga.gh;
        g[n++] = ga.gR;
        const bool first = owned && c == 0;      // the adjoint in front of step 0 is the gradient of the series' prior
#pragma unroll
        for (int k = 0; k < D; ++k) g[n++] = first ? ad.l[k] : 0.0;
#pragma unroll
        for (int k = 0; k < DS; ++k) g[n++] = first ? ad.L[k] : 0.0;
    }
    if (owned) {
        dist_b = adjoint_distance<D>(ka.mc, ad, b1);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s += ::fabs(ad.l[k]) + ::fabs(b1.l[k]);
#pragma unroll
        for (int k = 0; k < DS; ++k) s += ::fabs(ad.L[k]) + ::fabs(b1.L[k]);
#pragma unroll
        for (int k = 0; k < NG; ++k) s += ::fabs(g[k]);
        finite = finite && (s < 1e300);
    }
    double lml = owned ? acc.total() : 0.0;
    finite = finite && (::fabs(lml) < 1e300);
    unsigned bits = 0;
    if (owned && !(dist_f <= ka.mc.tol)) bits |= 1u;
    if (owned && !(dist_b <= ka.mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lml += __shfl_xor(lml, off, 64);
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
        const double of = __shfl_xor(dist_f, off, 64), ob = __shfl_xor(dist_b, off, 64);
        dist_f = (of > dist_f) ? of : dist_f;
        dist_b = (ob > dist_b) ? ob : dist_b;
#pragma unroll
        for (int k = 0; k < NG; ++k) g[k] += __shfl_xor(g[k], off, 64);
    }
    if (lane == 0) {
        double* p = ka.part + (size_t)wave * AdjParts<D>::STRIDE;
        p[0] = lml;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
#pragma unroll
        for (int k = 0; k < NG; ++k) p[4 + k] = g[k];
    }
}

// The adjoint gradient of an SDE-described model: k_sweep_adjoint's skeleton with the transitions built from the gaps and the sums over
// (lam, N1, N2, Pinf) in place of (A, Q).  part[wave]: [lml, bits, dist_f, dist_b | gl d | gN1 d*d | gN2 d*d | gPinf packed | ga d | gH d | sum gh_t |
// sum gR_t | gA1 d*d | gx0m d | gx0P packed].  d = 4: the gl and gN2 sums of a lane sit in LDS behind the block's states (SdeSums).
template <int D> struct AdjPartsSde {
    static constexpr int NG = AdjAccSde<D>::N + D * D + SD<D>::NS, STRIDE = 4 + NG;
};

template <int D, int XS>
__global__ __launch_bounds__(64, 1) void k_sweep_adjoint_sde(const AArgs<D> by_value) {
    (void)by_value;
    const AArgs<D>& ar = *(const AArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();
    const KArgs<D>& ka = ar.ka;
    constexpr int B = SdeSums<D>::B, NS = SD<D>::NS, DS = SD<D>::DS;
    constexpr bool LDS = SdeSums<D>::LDS;
    constexpr int NL = SdeSums<D>::NL;
    __shared__ double sF[B * NS * 64];      // the block's filtering states
    __shared__ double sS[LDS ? NL * 64 : 1];      // (d = 4) the lanes' gl and gN2 sums
    __shared__ double sA1[D * D];           // G_0 of the series' first step (one lane of wave 0)
    const int lane = threadIdx.x;
    const long long wave = blockIdx.x;
    const long long T = ka.T;
    const int C = ka.C;
    const long long c = wave * kOwned + lane - 1;
    const bool active = c >= 0 && c < ka.nchunks;
    const long long t0 = active ? c * C : 0;
    long long t1 = active ? t0 + C : 0;
    t1 = t1 < T ? t1 : (active ? T : 0);
    const long long t1r = (t1 + 7) & ~7ll;
    const bool runs = active && lane >= 1;
    const bool owned = runs && lane <= kOwned;
    bool ok = true;

    if constexpr (LDS) {
#pragma unroll
        for (int k = 0; k < NL; ++k) sS[k * 64 + lane] = 0.0;
    }
    if (lane < D * D) sA1[lane] = 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    ModelR<D, true> mr;
    mr.init(ka.mc);
    State<D> gen, x0;
    set_state<D>(gen, ka.mc.gm, ka.mc.gP);
    set_state<D>(x0, ka.mc.x0m, ka.mc.x0P);
    double* ck = ka.ckpt + (size_t)wave * (size_t)(C / B) * NS * 64;

    // ---- forwards: the warm-up over the chunk's last W steps, the shift, the chunk with its checkpoints
    State<D> x, e1;
    LmlAcc acc;
    {
        const long long tw = t1r - ka.W;
        x = tw <= 0 ? x0 : gen;
        for (int seg = 0; seg < 2; ++seg) {      // (ONE call site for both runs: the loop body exists once)
            const bool warm = seg == 0;
            forward_run<D, true, XS, B>(ka, mr, warm ? tw : t0, warm ? ka.W / B : C / B, warm ? (tw > 0 ? tw : 0) : t0, warm ? t1r : (runs ? t1r : t0), x, acc, !warm,
                                        warm ? (double*)nullptr : ck, lane, ok);
            if (warm) {
                e1 = x;
#pragma unroll
                for (int k = 0; k < D; ++k) x.m[k] = shfl_up1(e1.m[k]);
#pragma unroll
                for (int k = 0; k < DS; ++k) x.P[k] = shfl_up1(e1.P[k]);
                if (t0 == 0) x = x0;
                acc = LmlAcc();
            }
        }
    }
    double dist_f = 0.0, dist_b = 0.0;
    bool finite = true;
    if (owned) {
        dist_f = state_distance<D>(ka.mc, x, e1);
        finite = state_finite<D>(x) && state_finite<D>(e1);
    }

    // ---- backwards, the warm-up: the adjoint in front of the chunk's first step as its first Wa steps give it from zero
    Adj<D> b1;
    b1.zero();
    {
        const long long te = (t0 + ka.Wb < t1) ? t0 + ka.Wb : t1;
        adjoint_run_sde<D, XS, B, false>(ka, mr, t0, ka.Wb / B, runs ? te : t0, b1, (AdjAccSde<D>*)nullptr, (double*)nullptr, (double*)nullptr, (double*)nullptr,
                                         (double*)nullptr, ck, sF, lane, ok);
    }
    // ---- backwards, the chunk: from the next lane's adjoint in front of ITS first step (zero behind the series' last step)
    Adj<D> ad;
#pragma unroll
    for (int k = 0; k < D; ++k) ad.l[k] = shfl_dn1(b1.l[k]);
#pragma unroll
    for (int k = 0; k < DS; ++k) ad.L[k] = shfl_dn1(b1.L[k]);
    if (t1 == T) ad.zero();
    AdjAccSde<D> ga;
    ga.zero();
    adjoint_run_sde<D, XS, B, true>(ka, mr, t0, C / B, owned ? t1 : t0, ad, &ga, sS + lane, sA1, ar.gh_steps, ar.gR_steps, ck, sF, lane, ok);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();

    // ---- the wave's share: fixed-order sums over the lanes
    constexpr int NG = AdjPartsSde<D>::NG;
    double g[NG];
    {
        int n = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) g[n++] = LDS ? sS[(LDS ? k : 0) * 64 + lane] : ga.gl[k];
#pragma unroll
        for (int k = 0; k < D * D; ++k) g[n++] = ga.gN1[k];
#pragma unroll
        for (int k = 0; k < D * D; ++k) g[n++] = LDS ? sS[(LDS ? D + k : 0) * 64 + lane] : ga.gN2[k];
#pragma unroll
        for (int k = 0; k < DS; ++k) g[n++] = ga.gPinf[k];
#pragma unroll
        for (int k = 0; k < D; ++k) g[n++] = ga.ga[k];
#pragma unroll
        for (int k = 0; k < D; ++k) g[n++] = ga.gH[k];
        g[n++] = ga.gh;
        g[n++] = ga.gR;
        const bool first = owned && c == 0;      // the adjoint in front of step 0 is the gradient of the series' prior
#pragma unroll
        for (int k = 0; k < D * D; ++k) g[n++] = first ? sA1[k] : 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) g[n++] = first ? ad.l[k] : 0.0;
#pragma unroll
        for (int k = 0; k < DS; ++k) g[n++] = first ? ad.L[k] : 0.0;
    }
    if (owned) {
        dist_b = adjoint_distance<D>(ka.mc, ad, b1);
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) s += ::fabs(ad.l[k]) + ::fabs(b1.l[k]);
#pragma unroll
        for (int k = 0; k < DS; ++k) s += ::fabs(ad.L[k]) + ::fabs(b1.L[k]);
#pragma unroll
        for (int k = 0; k < NG; ++k) s += ::fabs(g[k]);
        finite = finite && (s < 1e300);
    }
    double lml = owned ? acc.total() : 0.0;
    finite = finite && (::fabs(lml) < 1e300);
    unsigned bits = 0;
    if (owned && !(dist_f <= ka.mc.tol)) bits |= 1u;
    if (owned && !(dist_b <= ka.mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        lml += __shfl_xor(lml, off, 64);
        bits |= (unsigned)__shfl_xor((int)bits, off, 64);
        const double of = __shfl_xor(dist_f, off, 64), ob = __shfl_xor(dist_b, off, 64);
        dist_f = (of > dist_f) ? of : dist_f;
        dist_b = (ob > dist_b) ? ob : dist_b;
#pragma unroll
        for (int k = 0; k < NG; ++k) g[k] += __shfl_xor(g[k], off, 64);
    }
    if (lane == 0) {
        double* p = ka.part + (size_t)wave * AdjPartsSde<D>::STRIDE;
        p[0] = lml;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
#pragma unroll
        for (int k = 0; k < NG; ++k) p[4 + k] = g[k];
    }
}

// ------------------------------------------------------------------------------------------------------------------------ host side
struct Engine {
    Plan p;
    Forced forced;
    double* part = nullptr;             // pinned: the waves' shares
    size_t part_cap = 0;
    int part_stride = 4;                // doubles per wave in `part`: 4, and the gradient's sums behind them in an adjoint call
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
void force_geometry(Engine* e, int C, int W, int Wb, int Wd, int Wa) {
    e->forced.C = C;
    e->forced.W = W;
    e->forced.Wb = Wb;
    e->forced.Wd = Wd;
    e->forced.Wa = Wa;
}
void geometry(const Engine* e, int* C, int* W, int* Wb, int64_t* nwaves, int* Wd) {
    if (C) *C = e->p.C;
    if (W) *W = e->p.W;
    if (Wb) *Wb = e->p.Wb;
    if (nwaves) *nwaves = e->p.nwaves;
    if (Wd) *Wd = e->p.Wd;
}
bool plan(Engine* e, const ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, std::string* why, int wd_hint, int wa_hint) {
    return make_plan(&e->p, e->forced, m, T, w_hint, wb_hint, num_cu, why, wd_hint, wa_hint);
}

namespace {

template <int D> void fill_args(const Engine* e, const Call& c, KArgs<D>& ka) {
    std::memcpy(&ka.mc, e->p.mc, sizeof ka.mc);
    ka.st.y = c.y;
    ka.st.mask = c.mask;
    ka.st.R = c.R;
    ka.st.hh = c.hh;
    ka.st.tau = c.tau;
    ka.st.Rnew = c.Rnew;
    ka.st.rnew_per_step = c.rnew_per_step;
    ka.T = c.T;
    ka.C = e->p.C;
    ka.W = e->p.W;
    ka.Wb = e->p.Wb;
    ka.nchunks = e->p.nchunks;
    ka.mean = c.mean;
    ka.var = c.var;
    ka.ckpt = static_cast<double*>(e->ckpt);
    ka.part = e->part;
}
template <int D, bool SDE, int XS, bool POST> void launch(Engine* e, hipStream_t stream, const Call& c) {
    KArgs<D> ka;
    fill_args<D>(e, c, ka);
    hipLaunchKernelGGL((k_sweep<D, SDE, XS, POST>), dim3((unsigned)e->p.nwaves), dim3(64), 0, stream, ka);
}
template <int D, bool SDE, int XS> void launch_draw(Engine* e, hipStream_t stream, const Call& c) {
    DArgs<D> ar;
    fill_args<D>(e, c, ar.ka);
    ar.ka.Wb = e->p.Wd;      // (the kernel's second warm-up is the draw's)
    ar.da.eps_t = c.eps_t;
    ar.da.eps_e = c.eps_e;
    for (int k = 0; k < 4; ++k) ar.da.eps_0[k] = c.eps_0[k];
    ar.da.y_out = c.y_out;
    hipLaunchKernelGGL((k_sweep_draw<D, SDE, XS>), dim3((unsigned)e->p.nwaves), dim3(64), 0, stream, ar);
}

template <int D, int XS> void launch_adjoint(Engine* e, hipStream_t stream, const Call& c) {
    AArgs<D> ar;
    fill_args<D>(e, c, ar.ka);
    ar.ka.Wb = e->p.Wa;      // (the kernel's second warm-up is the adjoint's)
    ar.gh_steps = c.gh_steps;
    ar.gR_steps = c.gR_steps;
    hipLaunchKernelGGL((k_sweep_adjoint<D, XS>), dim3((unsigned)e->p.nwaves), dim3(64), 0, stream, ar);
}

template <int D, int XS> void launch_adjoint_sde(Engine* e, hipStream_t stream, const Call& c) {
    AArgs<D> ar;
    fill_args<D>(e, c, ar.ka);
    ar.ka.Wb = e->p.Wa;
    ar.gh_steps = c.gh_steps;
    ar.gR_steps = c.gR_steps;
    hipLaunchKernelGGL((k_sweep_adjoint_sde<D, XS>), dim3((unsigned)e->p.nwaves), dim3(64), 0, stream, ar);
}

template <int D, bool SDE, int XS> void launch_x(Engine* e, hipStream_t stream, const Call& c) {
    if (c.adjoint) {
        if constexpr (SDE) launch_adjoint_sde<D, XS>(e, stream, c);
        else launch_adjoint<D, XS>(e, stream, c);
    } else if (c.y_out != nullptr) launch_draw<D, SDE, XS>(e, stream, c);
    else if (c.mean != nullptr) launch<D, SDE, XS, true>(e, stream, c);
    else launch<D, SDE, XS, false>(e, stream, c);
}
template <int D, bool SDE> void launch_s(Engine* e, hipStream_t stream, const Call& c) {
    const int xs = (c.R != nullptr ? 1 : 0) | (c.hh != nullptr ? 2 : 0);
    switch (xs) {
        case 0: launch_x<D, SDE, 0>(e, stream, c); break;
        case 1: launch_x<D, SDE, 1>(e, stream, c); break;
        case 2: launch_x<D, SDE, 2>(e, stream, c); break;
        default: launch_x<D, SDE, 3>(e, stream, c); break;
    }
}
template <int D> void launch_d(Engine* e, hipStream_t stream, const Call& c) {
    if (e->p.sde) launch_s<D, true>(e, stream, c);
    else launch_s<D, false>(e, stream, c);
}

}  // namespace

const char* kernel_name(int, bool sde, bool post, bool draw) {
    if (draw) return sde ? "k_sweep_draw<sde>" : "k_sweep_draw<lti>";
    return sde ? (post ? "k_sweep<sde,posterior>" : "k_sweep<sde,logpdf>") : (post ? "k_sweep<lti,posterior>" : "k_sweep<lti,logpdf>");
}

const char* adjoint_kernel_name() { return "k_sweep_adjoint<lti>"; }
const char* adjoint_sde_kernel_name() { return "k_sweep_adjoint<sde>"; }

int enqueue(Engine* e, hipStream_t stream, const Call& c, const char** kname, std::string* err) {
    auto fail = [&](const char* what, hipError_t rc) {
        if (err) *err = std::string(what) + ": " + hipGetErrorString(rc);
        return 1;
    };
    const Plan& p = e->p;
    const bool draw = c.y_out != nullptr;
    const bool post = c.mean != nullptr || draw || c.adjoint;      // (the draw and the adjoint keep the posterior call's checkpoints)
    if (c.adjoint && (draw || c.mean != nullptr)) {
        if (err) *err = "k_sweep_adjoint: no other output in the call";
        return 1;
    }
    const int NS = p.d + p.d * (p.d + 1) / 2;
    e->part_stride = c.adjoint ? 4 + (p.d * p.d + 2 * p.d + (NS - p.d) + 2) + NS : 4;      // (AdjParts<d>::STRIDE: 4, AdjAcc<d>::N, an adjoint)
    if (c.adjoint && p.sde) e->part_stride = 4 + (3 * p.d + 2 * p.d * p.d + (NS - p.d) + 2) + p.d * p.d + NS;      // (AdjPartsSde<d>::STRIDE)
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
    if (post) {
        const int B = (c.adjoint && p.sde) ? sde_adjoint_block(p.d) : (p.d <= 3 ? 8 : 4);
        const size_t need = (size_t)p.nwaves * (size_t)(p.C / B) * NS * 64 * sizeof(double);
        if (need > e->ckpt_cap) {
            if (e->ckpt) (void)tgp_alloc::dev_free(e->ckpt);
            e->ckpt = nullptr;
            e->ckpt_cap = 0;
            hipError_t rc = tgp_alloc::dev_malloc(&e->ckpt, need);
            if (rc != hipSuccess) return fail("hipMalloc", rc);
            e->ckpt_cap = need;
        }
    }
    if (draw && (c.eps_t == nullptr || c.eps_e == nullptr || c.Rnew == nullptr)) {
        if (err) *err = "k_sweep_draw: a draw needs eps_t, eps_e and Rnew";
        return 1;
    }
    if (kname) *kname = c.adjoint ? (p.sde ? adjoint_sde_kernel_name() : adjoint_kernel_name()) : kernel_name(p.d, p.sde, post, draw);
    switch (p.d) {
        case 1: launch_d<1>(e, stream, c); break;
        case 2: launch_d<2>(e, stream, c); break;
        case 3: launch_d<3>(e, stream, c); break;
        default: launch_d<4>(e, stream, c); break;
    }
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return fail("k_sweep launch", rc);
    return 0;
}

double finish(Engine* e, int* status, int* w, int* wb, double* dist_f, double* dist_b, int* wd, int* wa) {
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
    if (wd) *wd = e->p.Wd;
    if (wa) *wa = e->p.Wa;
    if (dist_f) *dist_f = df;
    if (dist_b) *dist_b = db;
    return lml;
}

void adjoint_blocks(const Engine* e, const AdjointOut& o) { adjoint_blocks_from_parts(e->part, e->p.nwaves, e->part_stride, e->p.d, o); }

void adjoint_blocks_sde(const Engine* e, const AdjointSdeOut& o) {
    const int d = e->p.d, dd = d * d, ds = d * (d + 1) / 2, ng = e->part_stride - 4;
    std::vector<double> g((size_t)ng, 0.0);
    for (int64_t i = 0; i < e->p.nwaves; ++i) {      // fixed order: two calls on the same series give the same bits
        const double* q = e->part + (size_t)i * e->part_stride + 4;
        for (int k = 0; k < ng; ++k) g[(size_t)k] += q[k];
    }
    const double *gl = g.data(), *gN1 = gl + d, *gN2 = gN1 + dd, *gPi = gN2 + dd, *ga = gPi + ds, *gH = ga + d, *gs = gH + d, *gA1 = gs + 2, *gm = gA1 + dd,
                 *gP = gm + d;
    auto unpack = [d](const double* packed, double* full) {
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) full[i + j * d] = packed[pidx(i, j)];
    };
    std::memcpy(o.gl, gl, sizeof(double) * d);
    std::memcpy(o.gN1, gN1, sizeof(double) * dd);
    std::memcpy(o.gN2, gN2, sizeof(double) * dd);
    unpack(gPi, o.gPinf);
    std::memcpy(o.ga, ga, sizeof(double) * d);
    std::memcpy(o.gH, gH, sizeof(double) * d);
    *o.ghh = gs[0];
    *o.gR = gs[1];
    std::memcpy(o.gA1, gA1, sizeof(double) * dd);
    std::memcpy(o.gx0m, gm, sizeof(double) * d);
    unpack(gP, o.gx0P);
}

}  // namespace tgp_sweep
