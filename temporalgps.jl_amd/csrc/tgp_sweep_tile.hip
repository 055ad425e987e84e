// The tile sweep: see tgp_sweep_tile.hpp (what and why) and DESIGN 4.16 (geometry, operand layouts, LDS and register budget, the record).  gfx950 only.
// One wave per workgroup; a wave's LDS: one padded 16 x 17 tile (2176 B), the transpose of A P (forwards) and of A' N (backwards); the adjoint and the
// draw keep the eight filtering states of a block beside it.
//
// Layouts of v_mfma_f64_16x16x4_f64 as tgp_dense_fused.hpp uses them, lane = (lr = lane % 16, lq = lane / 16):
//   A-operand (16 x 4):  lane holds X[lr][lq]         B-operand (4 x 16):  lane holds Y[lq][lr]
//   accumulator (16 x 16, 4 doubles):  register r of a lane holds Z[lq + 4 r][lr]
// so register r of an accumulator-layout tile S is the B-operand "rows lq + 4 r of S", and with xf[r] = X[lr][lq + 4 r] the four MFMAs
// sum_r mfma(xf[r], S[r]) give X S: the k-index of the product runs over lq + 4 r in another order, nothing else.
// A vector lives in "column form" (lane holds v[lr], the same in the four row groups); its "row form" v[lq + 4 r] comes by four shuffles.
// The padding (rows and columns >= d) is zero in every block of the model, stays zero in P, m, N, r and adds exact zeros to every sum.
#include "tgp_sweep_tile.hpp"
#include "tgp_alloc.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace tgp_sweep_tile {

using tgp_sweep::fast_rcp;
using tgp_sweep::LmlAcc;
using tgp_sweep::TileModelC;

typedef double d4 __attribute__((ext_vector_type(4)));

constexpr int DP = tgp_sweep::kTileDP, REC = tgp_sweep::kTileRec;
constexpr int kTLD = DP + 1;      // the transpose tile's leading dimension: rows written by 16 consecutive lanes, columns read at stride 17
// The adjoint call.  kAdjB: steps between two checkpoints = states of a block recomputed into LDS: 8 x 2176 B beside the transpose tile's
// 2176 B are 19 584 B, within the 20 480 B that keep eight workgroups on a CU (9 states would be 21 760 B).
constexpr int kAdjB = 8;
constexpr int kAdjState = DP * DP + DP;                  // a filtering state: P in the accumulator layout [r][lane], then m
constexpr int kAdjSums = 3 * DP * DP + 3 * DP + 2;      // a wave's record: gA | gQ | gx0P (16 x 16, [i + 16 j]) | ga | gH | gx0m (16) | sum gh_t | sum gR_t

struct TArgs {
    const TileModelC* mc;      // device
    tgp_sweep::Streams st;
    long long T;
    int C, W, Wb, d;
    double* mean;
    double* var;
    double* rec;       // [chunk][C + Wb][REC]: the forward run's record of the chunk's steps and of the Wb steps behind them (posterior calls)
    double* part;      // [chunk][4]: share of the log marginal likelihood, status bits, forward / backward distance (pinned host memory)
    // an adjoint call (k_sweep_tile_adjoint; Wb carries the adjoint's warm-up Wa)
    double* gh;        // [T] or null: d logpdf / d h_t, d logpdf / d R_t of every step
    double* gR;
    double* ckpt;      // [chunk][(C + Wa) / kAdjB][kAdjState]: the filtering state in front of every kAdjB-th step of the chunk and of the Wa steps behind it
    double* sums;      // [chunk][kAdjSums]: the wave's sums of the block gradients
};

__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
template <int CTRL> __device__ __forceinline__ double dpp_move(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// sum over the 16 lanes of a row (one DPP row), every lane ending with the same bits
__device__ __forceinline__ double row_sum(double x) {
    x += dpp_move<0xB1>(x);       // quad_perm:[1,0,3,2]
    x += dpp_move<0x4E>(x);       // quad_perm:[2,3,0,1]
    x += dpp_move<0x141>(x);      // row_half_mirror
    x += dpp_move<0x140>(x);      // row_mirror
    return x;
}
// sum over the four row groups (lanes lr, lr + 16, lr + 32, lr + 48), every lane ending with the same bits
__device__ __forceinline__ double cross_sum(double x) {
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    return x;
}
__device__ __forceinline__ double wave_max(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double o = __shfl_xor(x, off, 64);
        x = o > x ? o : x;
    }
    return x;
}
__device__ __forceinline__ double rdlane(double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l), hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ d4 mfma(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }

// a lane's view of the wave's tile
struct Lane {
    int lr, lq;
    double* sT;        // the wave's transpose tile

    // X S X' + init for a symmetric S in the accumulator layout, xf[r] = X[lr][lq + 4 r]: T = X S (four MFMAs), T' through LDS, X T' on top of init
    __device__ __forceinline__ d4 sandwich(const d4& xf, const d4& S, const d4& init) const {
        d4 t = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 4; ++r) t = mfma(xf[r], S[r], t);
        wave_sync();
#pragma unroll
        for (int r = 0; r < 4; ++r) sT[(lq + 4 * r) * kTLD + lr] = t[r];
        wave_sync();
        d4 out = init;
#pragma unroll
        for (int r = 0; r < 4; ++r) out = mfma(xf[r], sT[lr * kTLD + lq + 4 * r], out);
        return out;
    }
    // (X v)[lr] in column form from v in column form
    __device__ __forceinline__ double matvec(const d4& xf, double vC) const {
        double p = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) p = fma(xf[r], __shfl(vC, lq + 4 * r, 64), p);
        return cross_sum(p);
    }
    // S v for a symmetric S in the accumulator layout: row form (register r: element lq + 4 r) by row sums, column form by symmetry
    __device__ __forceinline__ void symvec(const d4& S, double vC, const d4& vR, d4& outR, double& outC) const {
        double p = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            outR[r] = row_sum(S[r] * vC);
            p = fma(S[r], vR[r], p);
        }
        outC = cross_sum(p);
    }
};

// the blocks of the model a lane keeps in registers
struct Blocks {
    d4 af;         // A[lr][lq + 4 r]: the A-operands of the forward sandwich
    d4 atf;        // A[lq + 4 r][lr]: those of the backward one (A')
    d4 Q;          // accumulator layout
    d4 HR;         // H in row form
    double HC, aC; // H, a in column form
    double hh, R;
};

// 64 steps of the observation streams, one per lane (ascending from tb forwards, descending from tb backwards), handed out by v_readlane.
// XS bit 0: the noise variance is per step, bit 1: the emission offset is.
struct Row {
    double y, R, hh, rn;
    unsigned mk;
};
template <int XS, bool BACK> __device__ __forceinline__ void load_row(const TArgs& ka, long long tb, int lane, Row& r) {
    const long long t = tgp_sweep::clamp_t(BACK ? tb - lane : tb + lane, ka.T);
    r.y = BACK ? 0.0 : ka.st.y[t];
    r.R = ((XS & 1) && !BACK) ? ka.st.R[t] : 0.0;
    r.hh = (XS & 2) ? ka.st.hh[t] : 0.0;
    r.rn = BACK ? ka.st.Rnew[ka.st.rnew_per_step ? t : 0] : 0.0;
    r.mk = (!BACK && ka.st.mask != nullptr) ? (unsigned)ka.st.mask[t] : 0u;
}

// One step of the filter (lgc.jl:46-52, :247-257; a missing step predicts only).  rec (null: none): the step's record for the backward run.
__device__ __forceinline__ void fstep(const Lane& ln, const Blocks& b, d4& P, double& mC, double y, double Rt, double ht, bool obs, LmlAcc& acc, bool lml, bool& ok, double* rec) {
    const d4 Pm = ln.sandwich(b.af, P, b.Q);
    const double mp = ln.matvec(b.af, mC) + b.aC;
    d4 wR;
    double wC;
    ln.symvec(Pm, b.HC, b.HR, wR, wC);
    const double hph = row_sum(b.HC * wC), hm = row_sum(b.HC * mp);
    const double S = obs ? hph + Rt : 1.0;
    ok = ok && (S > 0.0);
    const double iS = obs ? fast_rcp(S) : 0.0;
    const double v = obs ? (y - (hm + ht)) : 0.0;
    const double viS = v * iS;
    mC = fma(wC, viS, mp);
    const double wi = wC * iS;
#pragma unroll
    for (int r = 0; r < 4; ++r) P[r] = fma(-wR[r], wi, Pm[r]);
    if (lml) {
        acc.q = fma(v, viS, acc.q);
        acc.prod *= S;
        acc.n += obs ? 1.0 : 0.0;
    }
    if (rec != nullptr) {
        if (ln.lq == 0) rec[ln.lr] = wC;
        if (ln.lr == 0 && ln.lq == 1) {
            rec[DP] = hph;
            rec[DP + 1] = hm;
            rec[DP + 2] = v;
            rec[DP + 3] = obs ? S : 0.0;
        }
    }
}

// One step of the Bryson-Frazier recursion, backwards over step t with its record: (r, N) behind the step on entry, in front of it on return --
// m_s = m- + P- r, P_s = P- - P- N P- -- and the step's marginals without the replaced noise: mean = H m- + w' r + h_t, var = H P- H' - w' N w.
__device__ __forceinline__ void bstep(const Lane& ln, const Blocks& b, d4& N, double& rC, const double* rec, double ht, double& mean, double& var) {
    const double wC = rec[ln.lr];
    d4 wR;
#pragma unroll
    for (int r = 0; r < 4; ++r) wR[r] = rec[ln.lq + 4 * r];
    const double hph = rec[DP], hm = rec[DP + 1], v = rec[DP + 2], s = rec[DP + 3];
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    const d4 Np = ln.sandwich(b.atf, N, zero);      // A' N A
    const double rp = ln.matvec(b.atf, rC);         // A' r
    d4 uR;
    double uC;
    ln.symvec(Np, wC, wR, uR, uC);                  // u = (A' N A) w
    const double q = row_sum(wC * uC), rho = row_sum(wC * rp);
    const double iS = s > 0.0 ? fast_rcp(s) : 0.0;  // (a missing step: (r, N) pass through the transition alone)
    const double c = fma(-hph, iS, 1.0);            // 1 - H K = R / s
    mean = fma(rho, c, hph * v * iS) + (hm + ht);
    var = fma(-q * c, c, hph * c);
    rC = fma(b.HC, (v - rho) * iS, rp);
    const double k2 = fma(q * iS, iS, iS);
#pragma unroll
    for (int r = 0; r < 4; ++r) N[r] = fma(b.HR[r] * b.HC, k2, fma(-iS, fma(b.HR[r], uC, uR[r] * b.HC), Np[r]));
}

// (two waves per SIMD: the register counts are in profiles/sweep_tile_resources.txt)
template <int XS, bool POST>
__global__ __launch_bounds__(64) void k_sweep_tile(const TArgs ka) {
    __shared__ double sT[DP * kTLD];
    const int lane = threadIdx.x;
    Lane ln;
    ln.lr = lane & 15;
    ln.lq = lane >> 4;
    ln.sT = sT;
    const int lr = ln.lr, lq = ln.lq;
    const TileModelC& mc = *ka.mc;
    Blocks b;
    d4 gP, x0P, sdR, isdR;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        b.af[r] = mc.A[DP * lr + i];
        b.atf[r] = mc.A[DP * i + lr];
        b.Q[r] = mc.Q[i + DP * lr];
        b.HR[r] = mc.H[i];
        gP[r] = mc.gP[i + DP * lr];
        x0P[r] = mc.x0P[i + DP * lr];
        sdR[r] = mc.sd[i];
        isdR[r] = mc.isd[i];
    }
    b.HC = mc.H[lr];
    b.aC = mc.a[lr];
    b.hh = mc.hh;
    b.R = mc.R;
    const double gmC = mc.gm[lr], x0mC = mc.x0m[lr], sdC = mc.sd[lr], isdC = mc.isd[lr];

    const long long T = ka.T, chunk = blockIdx.x;
    const long long t0 = chunk * ka.C, t1 = (t0 + ka.C < T) ? t0 + ka.C : T;
    double* const slab = POST ? ka.rec + (size_t)chunk * (size_t)(ka.C + ka.Wb) * REC : nullptr;
    bool ok = true, finite = true;
    double dist_f = 0.0, dist_b = 0.0;
    LmlAcc acc;

    // ---- forwards, four runs of the same loop.  0: the W steps in front of the chunk from the stationary prior (from the series' prior where they reach
    // step 0).  1: the chunk (record, log marginal likelihood).  2 (posterior calls): the Wb steps behind the chunk, record only.  3: the last W steps
    // of the chunk from the stationary prior -- what the NEXT wave starts from -- against run 1's end state.
    d4 P, Pend;
    double mC, mend;
    for (int run = 0; run < 4; ++run) {
        long long ta, tb;
        if (run == 0) { ta = t0 - ka.W; tb = t0; }
        else if (run == 1) { ta = t0; tb = t1; }
        else if (run == 2) { ta = t1; tb = POST ? ((t1 + ka.Wb < T) ? t1 + ka.Wb : T) : t1; }
        else { ta = t1 - ka.W; tb = t1 < T ? t1 : ta; }      // (the last chunk hands nothing over)
        if (run == 0 || run == 3) {
            const bool head = ta <= 0;      // the run reaches the series' first step: exact
#pragma unroll
            for (int r = 0; r < 4; ++r) P[r] = head ? x0P[r] : gP[r];
            mC = head ? x0mC : gmC;
            ta = head ? 0 : ta;
        }
        double* const rec = (POST && (run == 1 || run == 2)) ? slab : nullptr;
        Row in, nx;
        load_row<XS, false>(ka, ta, lane, in);
        for (long long tr = ta; tr < tb; tr += 64) {
            load_row<XS, false>(ka, tr + 64, lane, nx);      // in flight while this row computes (behind the last row: clamped, unused)
            const int n = (int)((tb - tr < 64) ? tb - tr : 64);
#pragma nounroll
            for (int k = 0; k < n; ++k) {
                const double y = rdlane(in.y, k);
                const double Rt = (XS & 1) ? rdlane(in.R, k) : b.R;
                const double ht = (XS & 2) ? rdlane(in.hh, k) : b.hh;
                const bool obs = __builtin_amdgcn_readlane((int)in.mk, k) == 0;
                fstep(ln, b, P, mC, y, Rt, ht, obs, acc, run == 1, ok, rec != nullptr ? rec + (size_t)(tr + k - t0) * REC : nullptr);
                if (run == 1 && (k & 7) == 7) acc.flush();
            }
            if (run == 1) acc.flush();
            in = nx;
        }
        if (run == 1) {
            Pend = P;
            mend = mC;
        }
        if (run == 3 && t1 < T) {
            double worst = (lr < ka.d) ? ::fabs(mend - mC) / (sdC + ::fabs(mend) + ::fabs(mC)) : 0.0, s = ::fabs(mend) + ::fabs(mC);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double e = ::fabs(Pend[r] - P[r]) * (isdR[r] * isdC);
                worst = e > worst ? e : worst;
                s += ::fabs(Pend[r]) + ::fabs(P[r]);
            }
            dist_f = wave_max(worst);
            finite = finite && (cross_sum(row_sum(s)) < 1e300);      // (false for NaN as well)
        }
    }

    if (POST) {
        // ---- backwards, three runs of the same loop.  0: the Wb steps behind the chunk from zero (exact where they reach the series' last step): the
        // (r, N) behind the chunk's last step.  1: the chunk, mean and variance of every step.  2: the chunk's own first Wb steps from zero -- what the
        // PREVIOUS wave continues from -- against run 1's result.
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");      // (the record is read back by other lanes)
        d4 N, Nown;
        double rC, rown;
        for (int run = 0; run < 3; ++run) {
            long long ta, tb;      // the steps tb - 1 .. ta
            if (run == 0) { ta = t1; tb = (t1 + ka.Wb < T) ? t1 + ka.Wb : T; }
            else if (run == 1) { ta = t0; tb = t1; }
            else { ta = t0; tb = t0 > 0 ? ((t0 + ka.Wb < t1) ? t0 + ka.Wb : t1) : t0; }      // (nobody continues from the first chunk)
            if (run != 1) {
#pragma unroll
                for (int r = 0; r < 4; ++r) N[r] = 0.0;
                rC = 0.0;
            }
            Row in, nx;
            load_row<XS, true>(ka, tb - 1, lane, in);
            for (long long tr = tb - 1; tr >= ta; tr -= 64) {
                load_row<XS, true>(ka, tr - 64, lane, nx);      // the next row: in flight through this one
                const int n = (int)((tr - ta + 1 < 64) ? tr - ta + 1 : 64);
                double om = 0.0, ov = 0.0;
#pragma nounroll
                for (int k = 0; k < n; ++k) {
                    const double ht = (XS & 2) ? rdlane(in.hh, k) : b.hh;
                    double mu, vr;
                    bstep(ln, b, N, rC, slab + (size_t)(tr - k - t0) * REC, ht, mu, vr);
                    om = (lane == k) ? mu : om;
                    ov = (lane == k) ? vr : ov;
                }
                if (run == 1 && lane < n) {
                    ka.mean[tr - lane] = om;
                    ka.var[tr - lane] = ov + in.rn;
                }
                in = nx;
            }
            if (run == 1) {
                Nown = N;
                rown = rC;
            }
            if (run == 2 && t0 > 0) {
                double worst = ::fabs(rown - rC) * sdC, s = ::fabs(rown) + ::fabs(rC);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const double e = ::fabs(Nown[r] - N[r]) * (sdR[r] * sdC);
                    worst = e > worst ? e : worst;
                    s += ::fabs(Nown[r]) + ::fabs(N[r]);
                }
                dist_b = wave_max(worst);
                finite = finite && (cross_sum(row_sum(s)) < 1e300);
            }
        }
    }

    // ---- the wave's share (every lane holds the same sums)
    const double lml = acc.total();
    finite = finite && (::fabs(lml) < 1e300);
    unsigned bits = 0;
    if (!(dist_f <= mc.tol)) bits |= 1u;
    if (POST && !(dist_b <= mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
    if (lane == 0) {
        double* p = ka.part + (size_t)chunk * 4;
        p[0] = lml;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
    }
}

// ---- the adjoint of the filter on the tile (the recursion: DESIGN 4.8, tests/_sweep_adjoint.py restated) ------------------------------
// A filtering state in LDS or in a checkpoint: every lane's four registers of P where it reads them back, m behind them (written by row group 0).
__device__ __forceinline__ void put_state(double* q, const Lane& ln, const d4& P, double mC) {
    const int lane = ln.lr + 16 * ln.lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) q[64 * r + lane] = P[r];
    if (ln.lq == 0) q[DP * DP + ln.lr] = mC;
}
__device__ __forceinline__ void get_state(const double* q, const Lane& ln, d4& P, double& mC) {
    const int lane = ln.lr + 16 * ln.lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) P[r] = q[64 * r + lane];
    mC = q[DP * DP + ln.lr];
}

// a wave's sums over its chunk: gA and gQ in the accumulator layout, ga and gH in column form
struct AdjSums {
    d4 gA, gQ;
    double ga, gH, gh, gR;
};

// One step of the adjoint, backwards over step t: (lam, Lam) = d logpdf / d (m, P) behind the step on entry, in front of it on return; (m, P): the
// filtering state in front of the step.  A missing step (iS = 0, v = 0) passes the adjoint through the transition alone and leaves zeros in gh, gR.
// sum: the step belongs to the wave's chunk (the warm-up walks add nothing).  20 MFMAs with `sum`, 16 without.
__device__ __forceinline__ void astep(const Lane& ln, const Blocks& b, const d4& P, double mC, double y, double Rt, double ht, bool obs, d4& Lam, double& lamC,
                                      AdjSums& s, bool sum, double& gh, double& gR) {
    const int lr = ln.lr, lq = ln.lq;
    d4 AP = {0.0, 0.0, 0.0, 0.0};      // A P: register r is the B-operand "rows lq + 4 r of A P" of the gA product below
#pragma unroll
    for (int r = 0; r < 4; ++r) AP = mfma(b.af[r], P[r], AP);
    wave_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) ln.sT[(lq + 4 * r) * kTLD + lr] = AP[r];
    wave_sync();
    d4 Pm = b.Q;                       // P- = A (A P)' + Q
#pragma unroll
    for (int r = 0; r < 4; ++r) Pm = mfma(b.af[r], ln.sT[lr * kTLD + lq + 4 * r], Pm);
    const double mp = ln.matvec(b.af, mC) + b.aC;
    d4 VR, LVR, lamR, VbR, Pb;
    double VC, LVC;
    ln.symvec(Pm, b.HC, b.HR, VR, VC);      // V = P- H'
    ln.symvec(Lam, VC, VR, LVR, LVC);       // Lam V
    const double S = obs ? row_sum(b.HC * VC) + Rt : 1.0;
    const double iS = obs ? fast_rcp(S) : 0.0;
    const double v = obs ? (y - (row_sum(b.HC * mp) + ht)) : 0.0;
    const double lV = row_sum(lamC * VC), VLV = row_sum(VC * LVC), viS = v * iS;
    const double vb = (lV - v) * iS;
    const double Sb = fma(fma(-lV, v, VLV) * iS, iS, -0.5 * fma(-viS, viS, iS));
    const double VbC = fma(Sb, b.HC, fma(lamC, viS, -2.0 * iS * LVC));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        lamR[r] = __shfl(lamC, lq + 4 * r, 64);
        VbR[r] = fma(Sb, b.HR[r], fma(lamR[r], viS, -2.0 * iS * LVR[r]));
        Pb[r] = fma(0.5, fma(VbR[r], b.HC, b.HR[r] * VbC), Lam[r]);      // Lam + (Vb H + H' Vb') / 2
    }
    gh = -vb;
    gR = Sb;
    const double mbC = fma(-vb, b.HC, lamC);      // lam - vb H'
    if (sum) {
        double pv = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) pv = fma(Pm[r], VbR[r], pv);
        s.gH += cross_sum(pv) + fma(Sb, VC, -vb * mp);      // P- Vb + Sb V - vb m-
        s.ga += mbC;
        s.gh += gh;
        s.gR += gR;
        // gA += mb m' + 2 Pb (A P): the symmetric Pb in the accumulator layout is its own A-operand (register r: Pb[lr][lq + 4 r])
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            s.gQ[r] += Pb[r];
            s.gA[r] = fma(fma(-vb, b.HR[r], lamR[r]), mC, s.gA[r]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) s.gA = mfma(2.0 * Pb[r], AP[r], s.gA);
    }
    const d4 zero = {0.0, 0.0, 0.0, 0.0};
    lamC = ln.matvec(b.atf, mbC);          // A' mb
    Lam = ln.sandwich(b.atf, Pb, zero);    // A' Pb A
}

// (two waves per SIMD: the register counts are in profiles/sweep_tile_adjoint_resources.txt)
template <int XS>
__global__ __launch_bounds__(64) void k_sweep_tile_adjoint(const TArgs ka) {
    __shared__ double sT[DP * kTLD];
    __shared__ double sX[kAdjB * kAdjState];      // the filtering states in front of a block's steps
    const int lane = threadIdx.x;
    Lane ln;
    ln.lr = lane & 15;
    ln.lq = lane >> 4;
    ln.sT = sT;
    const int lr = ln.lr, lq = ln.lq;
    const TileModelC& mc = *ka.mc;
    Blocks b;
    d4 gP, x0P, sdR, isdR;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        b.af[r] = mc.A[DP * lr + i];
        b.atf[r] = mc.A[DP * i + lr];
        b.Q[r] = mc.Q[i + DP * lr];
        b.HR[r] = mc.H[i];
        gP[r] = mc.gP[i + DP * lr];
        x0P[r] = mc.x0P[i + DP * lr];
        sdR[r] = mc.sd[i];
        isdR[r] = mc.isd[i];
    }
    b.HC = mc.H[lr];
    b.aC = mc.a[lr];
    b.hh = mc.hh;
    b.R = mc.R;
    const double gmC = mc.gm[lr], x0mC = mc.x0m[lr], sdC = mc.sd[lr], isdC = mc.isd[lr];

    const long long T = ka.T, chunk = blockIdx.x;
    const int Wa = ka.Wb;
    const long long t0 = chunk * ka.C, t1 = (t0 + ka.C < T) ? t0 + ka.C : T;
    const long long te = (t1 + Wa < T) ? t1 + Wa : T;      // the filter runs Wa steps beyond the chunk: the states of the adjoint's warm-up
    double* const slab = ka.ckpt + (size_t)chunk * (size_t)((ka.C + Wa) / kAdjB) * kAdjState;
    bool ok = true, finite = true;
    double dist_f = 0.0, dist_b = 0.0;
    LmlAcc acc;

    // ---- forwards: k_sweep_tile's four runs; runs 1 and 2 leave a checkpoint in front of every kAdjB-th step in place of the record
    d4 P, Pend;
    double mC, mend;
    for (int run = 0; run < 4; ++run) {
        long long ta, tb;
        if (run == 0) { ta = t0 - ka.W; tb = t0; }
        else if (run == 1) { ta = t0; tb = t1; }
        else if (run == 2) { ta = t1; tb = te; }
        else { ta = t1 - ka.W; tb = t1 < T ? t1 : ta; }
        if (run == 0 || run == 3) {
            const bool head = ta <= 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) P[r] = head ? x0P[r] : gP[r];
            mC = head ? x0mC : gmC;
            ta = head ? 0 : ta;
        }
        const bool keep = run == 1 || run == 2;
        Row in, nx;
        load_row<XS, false>(ka, ta, lane, in);
        for (long long tr = ta; tr < tb; tr += 64) {
            load_row<XS, false>(ka, tr + 64, lane, nx);
            const int n = (int)((tb - tr < 64) ? tb - tr : 64);
#pragma nounroll
            for (int k = 0; k < n; ++k) {
                const double y = rdlane(in.y, k);
                const double Rt = (XS & 1) ? rdlane(in.R, k) : b.R;
                const double ht = (XS & 2) ? rdlane(in.hh, k) : b.hh;
                const bool obs = __builtin_amdgcn_readlane((int)in.mk, k) == 0;
                const long long s = tr + k - t0;
                if (keep && (s & (kAdjB - 1)) == 0) put_state(slab + (size_t)(s / kAdjB) * kAdjState, ln, P, mC);
                fstep(ln, b, P, mC, y, Rt, ht, obs, acc, run == 1, ok, nullptr);
                if (run == 1 && (k & 7) == 7) acc.flush();
            }
            if (run == 1) acc.flush();
            in = nx;
        }
        if (run == 1) {
            Pend = P;
            mend = mC;
        }
        if (run == 3 && t1 < T) {
            double worst = (lr < ka.d) ? ::fabs(mend - mC) / (sdC + ::fabs(mend) + ::fabs(mC)) : 0.0, s = ::fabs(mend) + ::fabs(mC);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double e = ::fabs(Pend[r] - P[r]) * (isdR[r] * isdC);
                worst = e > worst ? e : worst;
                s += ::fabs(Pend[r]) + ::fabs(P[r]);
            }
            dist_f = wave_max(worst);
            finite = finite && (cross_sum(row_sum(s)) < 1e300);
        }
    }

    // ---- backwards, three walks of the same loop.  0: the Wa steps behind the chunk from a zero adjoint (exact where they reach the series' last step).
    // 1: the chunk, summing.  2: the chunk's own first Wa steps from zero -- what the PREVIOUS wave continues from -- against walk 1's result.
    // A walk goes over rows of 64 steps (the streams, one step per lane) and in a row over blocks of kAdjB steps: the block's states forwards from its
    // checkpoint into LDS, then the adjoint backwards over them.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");      // (a checkpoint's m is read back by other lanes)
    AdjSums sm;
    d4 Lam, Lown;
    double lamC = 0.0, lown = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) sm.gA[r] = sm.gQ[r] = Lam[r] = Lown[r] = 0.0;
    sm.ga = sm.gH = sm.gh = sm.gR = 0.0;
    for (int run = 0; run < 3; ++run) {
        long long ta, tb;      // the steps tb - 1 .. ta
        if (run == 0) { ta = t1; tb = te; }
        else if (run == 1) { ta = t0; tb = t1; }
        else { ta = t0; tb = t0 > 0 ? ((t0 + Wa < t1) ? t0 + Wa : t1) : t0; }      // (nobody continues from the first chunk)
        if (run != 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Lam[r] = 0.0;
            lamC = 0.0;
        }
        const long long nrow = (tb - ta + 63) / 64;
        Row in, nx;
        load_row<XS, false>(ka, ta + (nrow - 1) * 64, lane, in);
        for (long long j = nrow - 1; j >= 0; --j) {
            const long long tr = ta + j * 64;
            load_row<XS, false>(ka, tr - 64, lane, nx);      // the row walked next: in flight through this one (in front of the first: clamped, unused)
            const int n = (int)((tb - tr < 64) ? tb - tr : 64);
            double oh = 0.0, oR = 0.0;
            for (int k0 = ((n - 1) / kAdjB) * kAdjB; k0 >= 0; k0 -= kAdjB) {
                const int nb = (n - k0 < kAdjB) ? n - k0 : kAdjB;
                get_state(slab + (size_t)((tr + k0 - t0) / kAdjB) * kAdjState, ln, P, mC);
                bool okr = true;
#pragma nounroll
                for (int k = 0; k < nb; ++k) {
                    put_state(sX + k * kAdjState, ln, P, mC);
                    if (k + 1 < nb) {
                        const int kk = k0 + k;
                        fstep(ln, b, P, mC, rdlane(in.y, kk), (XS & 1) ? rdlane(in.R, kk) : b.R, (XS & 2) ? rdlane(in.hh, kk) : b.hh,
                              __builtin_amdgcn_readlane((int)in.mk, kk) == 0, acc, false, okr, nullptr);
                    }
                }
                wave_sync();
#pragma nounroll
                for (int k = nb - 1; k >= 0; --k) {
                    const int kk = k0 + k;
                    get_state(sX + k * kAdjState, ln, P, mC);
                    double gh, gR;
                    astep(ln, b, P, mC, rdlane(in.y, kk), (XS & 1) ? rdlane(in.R, kk) : b.R, (XS & 2) ? rdlane(in.hh, kk) : b.hh,
                          __builtin_amdgcn_readlane((int)in.mk, kk) == 0, Lam, lamC, sm, run == 1, gh, gR);
                    oh = (lane == kk) ? gh : oh;
                    oR = (lane == kk) ? gR : oR;
                }
                wave_sync();      // (the next block overwrites the slots)
            }
            if (run == 1 && lane < n) {
                if (ka.gh != nullptr) ka.gh[tr + lane] = oh;
                if (ka.gR != nullptr) ka.gR[tr + lane] = oR;
            }
            in = nx;
        }
        if (run == 1) {
            Lown = Lam;
            lown = lamC;
        }
        if (run == 2 && t0 > 0) {
            double worst = ::fabs(lown - lamC) * sdC, s = ::fabs(lown) + ::fabs(lamC);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double e = ::fabs(Lown[r] - Lam[r]) * (sdR[r] * sdC);
                worst = e > worst ? e : worst;
                s += ::fabs(Lown[r]) + ::fabs(Lam[r]);
            }
            dist_b = wave_max(worst);
            finite = finite && (cross_sum(row_sum(s)) < 1e300);
        }
    }

    // ---- the wave's record (device memory: k_sweep_tile_adjoint_sum adds the waves) and its share (pinned, every lane holds the same values)
    {
        double* q = ka.sums + (size_t)chunk * kAdjSums;
        const bool first = chunk == 0;      // the adjoint in front of step 0 is the gradient with respect to the prior
        double s = ::fabs(sm.ga) + ::fabs(sm.gH) + ::fabs(lown);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int at = (lq + 4 * r) + DP * lr;
            q[at] = sm.gA[r];
            q[DP * DP + at] = sm.gQ[r];
            q[2 * DP * DP + at] = first ? Lown[r] : 0.0;
            s += ::fabs(sm.gA[r]) + ::fabs(sm.gQ[r]) + ::fabs(Lown[r]);
        }
        if (lq == 0) {
            q[3 * DP * DP + lr] = sm.ga;
            q[3 * DP * DP + DP + lr] = sm.gH;
            q[3 * DP * DP + 2 * DP + lr] = first ? lown : 0.0;
        }
        if (lane == 0) {
            q[3 * DP * DP + 3 * DP] = sm.gh;
            q[3 * DP * DP + 3 * DP + 1] = sm.gR;
        }
        finite = finite && (cross_sum(row_sum(s)) < 1e300);
    }
    const double lml = acc.total();
    finite = finite && (::fabs(lml) < 1e300);
    unsigned bits = 0;
    if (!(dist_f <= mc.tol)) bits |= 1u;
    if (!(dist_b <= mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
    if (lane == 0) {
        double* p = ka.part + (size_t)chunk * 4;
        p[0] = lml;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
    }
}

// The waves' records added in index order, one entry per thread, into pinned host memory: no atomics, the same bits for the same geometry.
__global__ __launch_bounds__(64) void k_sweep_tile_adjoint_sum(const double* __restrict__ sums, long long nwaves, double* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= kAdjSums) return;
    double a = 0.0;
    for (long long w = 0; w < nwaves; ++w) a += sums[(size_t)w * kAdjSums + i];
    out[i] = a;
}

// ---- a draw from the posterior on the tile (the walk: tests/_sweepdraw.py draw_restated) ----------------------------------------------
// The draw's arguments beside TArgs (Wb carries the draw's warm-up Wd; ckpt: a chunk's checkpoints and, in the last slot, the state its filter ends on).
struct DArgs {
    TArgs t;
    const double* eps_t;      // [T][d]
    const double* eps_e;      // [T]
    double* y_out;            // [T]
    double eps_0[DP];         // the start, zero in the padding
};

// Right-looking Cholesky M + jit I_d + I_pad = U' U on an accumulator-layout tile, a pivot at a time (k is a compile-time index: row k sits in register
// k / 4 of row group k % 4).  Row k of U goes to every row group by two shuffles; the multipliers U[k][lq + 4 r] of a lane's own rows are that row in
// row form; rows above the pivot see zeros and stay.  U is never stored: what needs it is summed while its rows pass.
//   RHS:  the augmented right-hand side [B | c] (B a tile, c in column form) is forward-substituted in the same sweep: B <- Z = U^-T B in place,
//         q = U^-T c a scalar per pivot, g += Z' q.
//   else: nz += U' e for e in column form.
// The padding (k >= d) is the identity and meets zeros in B, c and e: skipped.  A pivot that is not positive clears ok.
template <bool RHS>
__device__ __forceinline__ void factor(const Lane& ln, int d, d4& M, double jit, d4& B, double& cC, double& gC, double eC, double& nzC, bool& ok) {
    const int lr = ln.lr, lq = ln.lq;
#pragma unroll
    for (int r = 0; r < 4; ++r) M[r] += (lq + 4 * r == lr) ? (lr < d ? jit : 1.0) : 0.0;
#pragma unroll
    for (int k = 0; k < DP; ++k) {
        const int kr = k >> 2, kq = k & 3;
        if (k < tgp_sweep::kTileMinD || k < d) {
            const double piv = rdlane(M[kr], k + 16 * kq);
            ok = ok && (piv > 0.0);
            const double is = 1.0 / ::sqrt(piv);
            double u = __shfl(M[kr], lr + 16 * kq, 64) * is;      // U[k][lr]
            u = lr < k ? 0.0 : u;
            double z = 0.0;
            if (RHS) {
                z = __shfl(B[kr], lr + 16 * kq, 64) * is;         // Z[k][lr]
                const double q = rdlane(cC, k) * is;
                cC = fma(-u, q, cC);
                gC = fma(z, q, gC);
            } else {
                nzC = fma(u, rdlane(eC, k), nzC);
            }
            if (k + 1 < DP) {
#pragma unroll
                for (int r = kr; r < 4; ++r) {
                    const double mu = __shfl(u, lq + 4 * r, 64);  // U[k][lq + 4 r]: zero in the rows above the pivot
                    M[r] = fma(-mu, u, M[r]);
                    if (RHS) B[r] = fma(-mu, z, B[r]);
                }
            }
            if (RHS) B[kr] = (lq == kq) ? z : B[kr];
        }
    }
}

// One step of the walk, backwards over step t: x = x_t on entry, x_(t-1) on return; (m, P): the filtering state in front of step t, e = eps_t[t] in
// column form.  With Z = U^-T (A P) and q = U^-T (x - m-), U'U = P- + 1e-10 I:  G (x - m-) = Z' q and L = P - Z' Z -- no back-substitution, no G.
// 12 MFMAs: A P, P- = A (A P)' + Q, and L = P - sum_r Z[r]' Z[r] on the registers Z sits in (register r is rows 4 r .. 4 r + 3 of Z: A- and B-operand at once).
__device__ __forceinline__ void dstep(const Lane& ln, const Blocks& b, int d, const d4& P, double mC, double eC, double& xC, bool& ok) {
    const int lr = ln.lr, lq = ln.lq;
    d4 Z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 4; ++r) Z = mfma(b.af[r], P[r], Z);      // A P
    wave_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) ln.sT[(lq + 4 * r) * kTLD + lr] = Z[r];
    wave_sync();
    d4 M = b.Q;
#pragma unroll
    for (int r = 0; r < 4; ++r) M = mfma(b.af[r], ln.sT[lr * kTLD + lq + 4 * r], M);
    double cC = xC - (ln.matvec(b.af, mC) + b.aC), gC = 0.0, nzC = 0.0;
    factor<true>(ln, d, M, 1e-10, Z, cC, gC, 0.0, nzC, ok);
    d4 L = P;
#pragma unroll
    for (int r = 0; r < 4; ++r) L = mfma(-Z[r], Z[r], L);
    factor<false>(ln, d, L, 1e-9, Z, cC, gC, eC, nzC, ok);      // (Z, c, g: not touched without a right-hand side)
    xC = mC + gC + nzC;
}

template <int XS>
__global__ __launch_bounds__(64) void k_sweep_tile_draw(const DArgs da) {
    __shared__ double sT[DP * kTLD];
    __shared__ double sX[kAdjB * kAdjState];      // the filtering states in front of a block's steps
    const TArgs& ka = da.t;
    const int lane = threadIdx.x;
    Lane ln;
    ln.lr = lane & 15;
    ln.lq = lane >> 4;
    ln.sT = sT;
    const int lr = ln.lr, lq = ln.lq, d = ka.d;
    const TileModelC& mc = *ka.mc;
    Blocks b;
    d4 gP, x0P, isdR;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = lq + 4 * r;
        b.af[r] = mc.A[DP * lr + i];
        b.atf[r] = 0.0;      // (the walk has no backward sandwich)
        b.Q[r] = mc.Q[i + DP * lr];
        b.HR[r] = mc.H[i];
        gP[r] = mc.gP[i + DP * lr];
        x0P[r] = mc.x0P[i + DP * lr];
        isdR[r] = mc.isd[i];
    }
    b.HC = mc.H[lr];
    b.aC = mc.a[lr];
    b.hh = mc.hh;
    b.R = mc.R;
    const double gmC = mc.gm[lr], x0mC = mc.x0m[lr], sdC = mc.sd[lr], isdC = mc.isd[lr];

    const long long T = ka.T, chunk = blockIdx.x;
    const int Wd = ka.Wb, nslots = (ka.C + Wd) / kAdjB;
    const long long t0 = chunk * ka.C, t1 = (t0 + ka.C < T) ? t0 + ka.C : T;
    const long long te = (t1 + Wd < T) ? t1 + Wd : T;      // the filter runs Wd steps beyond the chunk: the states of the walk's warm-up
    double* const slab = ka.ckpt + (size_t)chunk * (size_t)(nslots + 1) * kAdjState;
    bool ok = true, finite = true;
    double dist_f = 0.0, dist_b = 0.0;
    LmlAcc acc;

    // ---- forwards: k_sweep_tile_adjoint's four runs (the loop is repeated here: sharing it would move the existing kernels' code); the state behind
    // step te - 1 goes to the slab's last slot
    d4 P, Pend;
    double mC, mend;
    for (int run = 0; run < 4; ++run) {
        long long ta, tb;
        if (run == 0) { ta = t0 - ka.W; tb = t0; }
        else if (run == 1) { ta = t0; tb = t1; }
        else if (run == 2) { ta = t1; tb = te; }
        else { ta = t1 - ka.W; tb = t1 < T ? t1 : ta; }
        if (run == 0 || run == 3) {
            const bool head = ta <= 0;
#pragma unroll
            for (int r = 0; r < 4; ++r) P[r] = head ? x0P[r] : gP[r];
            mC = head ? x0mC : gmC;
            ta = head ? 0 : ta;
        }
        const bool keep = run == 1 || run == 2;
        Row in, nx;
        load_row<XS, false>(ka, ta, lane, in);
        for (long long tr = ta; tr < tb; tr += 64) {
            load_row<XS, false>(ka, tr + 64, lane, nx);
            const int n = (int)((tb - tr < 64) ? tb - tr : 64);
#pragma nounroll
            for (int k = 0; k < n; ++k) {
                const double y = rdlane(in.y, k);
                const double Rt = (XS & 1) ? rdlane(in.R, k) : b.R;
                const double ht = (XS & 2) ? rdlane(in.hh, k) : b.hh;
                const bool obs = __builtin_amdgcn_readlane((int)in.mk, k) == 0;
                const long long s = tr + k - t0;
                if (keep && (s & (kAdjB - 1)) == 0) put_state(slab + (size_t)(s / kAdjB) * kAdjState, ln, P, mC);
                fstep(ln, b, P, mC, y, Rt, ht, obs, acc, false, ok, nullptr);
            }
            in = nx;
        }
        if (run == 1) {
            Pend = P;
            mend = mC;
        }
        if (run == 2) put_state(slab + (size_t)nslots * kAdjState, ln, P, mC);
        if (run == 3 && t1 < T) {
            double worst = (lr < d) ? ::fabs(mend - mC) / (sdC + ::fabs(mend) + ::fabs(mC)) : 0.0, s = ::fabs(mend) + ::fabs(mC);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double e = ::fabs(Pend[r] - P[r]) * (isdR[r] * isdC);
                worst = e > worst ? e : worst;
                s += ::fabs(Pend[r]) + ::fabs(P[r]);
            }
            dist_f = wave_max(worst);
            finite = finite && (cross_sum(row_sum(s)) < 1e300);
        }
    }

    // ---- backwards, three walks of the same loop.  0: the Wd steps behind the chunk, from x = m_f behind them (from the true x_(T-1) where they reach the
    // series' end), on the real draws: the x behind the chunk's last step.  1: the chunk, y* of every step.  2: the chunk's own first Wd steps from
    // x = m_f -- what the PREVIOUS wave continues from -- against walk 1's x in front of the chunk.  A walk goes over rows of 64 steps and in a row over
    // blocks of kAdjB steps, as the adjoint's: the block's states forwards from its checkpoint into LDS, then the walk backwards over them.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "agent");      // (a checkpoint's m is read back by other lanes)
    double xC = 0.0, xown = 0.0, ysum = 0.0;
    for (int run = 0; run < 3; ++run) {
        long long ta, tb;      // the steps tb - 1 .. ta
        if (run == 0) { ta = t1; tb = te; }
        else if (run == 1) { ta = t0; tb = t1; }
        else { ta = t0; tb = t0 > 0 ? ((t0 + Wd < t1) ? t0 + Wd : t1) : t0; }      // (nobody continues from the first chunk)
        if (run == 2 && t0 == 0) break;
        if (run != 1) {      // the walk's start: the state behind step tb - 1
            get_state(slab + (size_t)(tb == te ? nslots : (tb - t0) / kAdjB) * kAdjState, ln, P, mC);
            xC = mC;
            if (tb == T) {      // x_(T-1) = m_f + chol(P_f + 1e-12 I).U' eps_0
                double c0 = 0.0, g0 = 0.0, nz = 0.0;
                d4 none = {0.0, 0.0, 0.0, 0.0};
                factor<false>(ln, d, P, 1e-12, none, c0, g0, da.eps_0[lr], nz, ok);
                xC = mC + nz;
            }
        }
        // eps_t[t] in column form, loaded a step ahead of its use
        auto load_e = [&](long long t) { return lr < d ? da.eps_t[(size_t)tgp_sweep::clamp_t(t, T) * d + lr] : 0.0; };
        double eC = load_e(tb - 1);
        const long long nrow = (tb - ta + 63) / 64;
        Row in, nx;
        load_row<XS, false>(ka, ta + (nrow - 1) * 64, lane, in);
        for (long long j = nrow - 1; j >= 0; --j) {
            const long long tr = ta + j * 64;
            load_row<XS, false>(ka, tr - 64, lane, nx);      // the row walked next: in flight through this one (in front of the first: clamped, unused)
            const int n = (int)((tb - tr < 64) ? tb - tr : 64);
            const long long tl = tgp_sweep::clamp_t(tr + lane, T);      // the lane's own step of the row: what rides with the output
            const double ee = da.eps_e[tl], rn = ka.st.Rnew[ka.st.rnew_per_step ? tl : 0];
            double oy = 0.0;
            for (int k0 = ((n - 1) / kAdjB) * kAdjB; k0 >= 0; k0 -= kAdjB) {
                const int nb = (n - k0 < kAdjB) ? n - k0 : kAdjB;
                get_state(slab + (size_t)((tr + k0 - t0) / kAdjB) * kAdjState, ln, P, mC);
                bool okr = true;
#pragma nounroll
                for (int k = 0; k < nb; ++k) {
                    put_state(sX + k * kAdjState, ln, P, mC);
                    if (k + 1 < nb) {
                        const int kk = k0 + k;
                        fstep(ln, b, P, mC, rdlane(in.y, kk), (XS & 1) ? rdlane(in.R, kk) : b.R, (XS & 2) ? rdlane(in.hh, kk) : b.hh,
                              __builtin_amdgcn_readlane((int)in.mk, kk) == 0, acc, false, okr, nullptr);
                    }
                }
                wave_sync();
#pragma nounroll
                for (int k = nb - 1; k >= 0; --k) {
                    const int kk = k0 + k;
                    const long long t = tr + kk;
                    const double hx = row_sum(b.HC * xC) + ((XS & 2) ? rdlane(in.hh, kk) : b.hh);      // H x_t + h_t
                    oy = (lane == kk) ? hx : oy;
                    const double en = load_e(t - 1);      // the next step's draws: in flight through this step
                    if (t > 0) {
                        get_state(sX + k * kAdjState, ln, P, mC);
                        dstep(ln, b, d, P, mC, eC, xC, ok);
                    }
                    eC = en;
                }
                wave_sync();      // (the next block overwrites the slots)
            }
            if (run == 1 && lane < n) {
                const double yo = fma(::sqrt(rn), ee, oy);
                da.y_out[tr + lane] = yo;
                ysum += ::fabs(yo);
            }
            in = nx;
        }
        if (run == 1) xown = xC;
        if (run == 2) {
            const double worst = (lr < d) ? ::fabs(xown - xC) / (sdC + ::fabs(xown) + ::fabs(xC)) : 0.0;
            dist_b = wave_max(worst);
        }
        finite = finite && (cross_sum(row_sum(::fabs(xC))) < 1e300);      // (false for NaN as well)
    }
    finite = finite && (cross_sum(row_sum(ysum)) < 1e300);

    unsigned bits = 0;
    if (!(dist_f <= mc.tol)) bits |= 1u;
    if (!(dist_b <= mc.tol_b)) bits |= 2u;
    if (!ok) bits |= 4u;
    if (!finite) bits |= 8u;
    if (lane == 0) {
        double* p = ka.part + (size_t)chunk * 4;
        p[0] = 0.0;
        p[1] = (double)bits;
        p[2] = dist_f;
        p[3] = dist_b;
    }
}

// ------------------------------------------------------------------------------------------------------------------------ host side
struct Engine {
    tgp_sweep::TilePlan p;
    tgp_sweep::Forced forced;
    double* part = nullptr;      // pinned: the waves' shares
    size_t part_cap = 0;
    void* mc = nullptr;          // device: the plan's TileModelC
    void* rec = nullptr;         // device: the posterior call's record
    size_t rec_cap = 0;
    void* ckpt = nullptr;        // device: the adjoint call's and the draw's checkpoints
    size_t ckpt_cap = 0;
    void* sums = nullptr;        // device: the adjoint call's records, one per wave
    size_t sums_cap = 0;
};

Engine* create() { return new Engine(); }
void destroy(Engine* e) {
    if (!e) return;
    if (e->part) (void)tgp_alloc::host_free(e->part);
    if (e->mc) (void)tgp_alloc::dev_free(e->mc);
    if (e->rec) (void)tgp_alloc::dev_free(e->rec);
    if (e->ckpt) (void)tgp_alloc::dev_free(e->ckpt);
    if (e->sums) (void)tgp_alloc::dev_free(e->sums);
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
    if (nwaves) *nwaves = e->p.nchunks;
}
bool plan(Engine* e, const tgp_sweep::ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, bool post, std::string* why) {
    return tgp_sweep::plan_tile(&e->p, e->forced, m, T, w_hint, wb_hint, num_cu, post, why);
}
const char* kernel_name(bool post) { return post ? "k_sweep_tile<posterior>" : "k_sweep_tile<logpdf>"; }
const char* adjoint_kernel_name() { return "k_sweep_tile_adjoint<lti>"; }
const char* draw_kernel_name() { return "k_sweep_tile_draw<lti>"; }

namespace {

// (the walk and, behind it on the stream, the sum of its records into the pinned block behind the waves' shares)
template <int XS> void launch_adjoint(const Engine* e, hipStream_t stream, const TArgs& ka) {
    hipLaunchKernelGGL((k_sweep_tile_adjoint<XS>), dim3((unsigned)e->p.nchunks), dim3(64), 0, stream, ka);
    hipLaunchKernelGGL(k_sweep_tile_adjoint_sum, dim3((kAdjSums + 63) / 64), dim3(64), 0, stream, ka.sums, (long long)e->p.nchunks,
                       e->part + (size_t)e->p.nchunks * 4);
}

template <int XS> void launch_draw(const Engine* e, hipStream_t stream, const DArgs& da) {
    hipLaunchKernelGGL((k_sweep_tile_draw<XS>), dim3((unsigned)e->p.nchunks), dim3(64), 0, stream, da);
}

template <int XS> void launch_x(const Engine* e, hipStream_t stream, const TArgs& ka, bool post) {
    if (post) hipLaunchKernelGGL((k_sweep_tile<XS, true>), dim3((unsigned)e->p.nchunks), dim3(64), 0, stream, ka);
    else hipLaunchKernelGGL((k_sweep_tile<XS, false>), dim3((unsigned)e->p.nchunks), dim3(64), 0, stream, ka);
}

}  // namespace

int enqueue(Engine* e, hipStream_t stream, const tgp_sweep::Call& c, const char** kname, std::string* err) {
    auto fail = [&](const char* what, hipError_t rc) {
        if (err) *err = std::string(what) + ": " + hipGetErrorString(rc);
        return 1;
    };
    const tgp_sweep::TilePlan& p = e->p;
    const bool post = c.mean != nullptr, draw = c.y_out != nullptr;
    if ((post || c.adjoint || draw) != p.post || (int)post + (int)c.adjoint + (int)draw > 1 || c.T != p.T || (post && (c.var == nullptr || c.Rnew == nullptr)) ||
        (draw && (c.Rnew == nullptr || c.eps_t == nullptr || c.eps_e == nullptr))) {
        if (err) *err = "k_sweep_tile: the call does not match its plan";
        return 1;
    }
    auto grow = [&](void** buf, size_t* cap, size_t need) {      // a device buffer of the engine's, at least `need` bytes
        if (need <= *cap) return hipSuccess;
        if (*buf) (void)tgp_alloc::dev_free(*buf);
        *buf = nullptr;
        *cap = 0;
        const hipError_t rc = tgp_alloc::dev_malloc(buf, need);
        if (rc == hipSuccess) *cap = need;
        return rc;
    };
    // (an adjoint call: the summed record sits behind the waves' shares in the same pinned block)
    const size_t need_part = ((size_t)p.nchunks * 4 + (c.adjoint ? kAdjSums : 0)) * sizeof(double);
    if (need_part > e->part_cap) {
        if (e->part) (void)tgp_alloc::host_free(e->part);
        e->part = nullptr;
        e->part_cap = 0;
        const size_t cap = std::max<size_t>(need_part, 1 << 16);
        hipError_t rc = tgp_alloc::host_malloc((void**)&e->part, cap, hipHostMallocDefault);
        if (rc != hipSuccess) return fail("hipHostMalloc", rc);
        e->part_cap = cap;
    }
    if (!e->mc) {
        hipError_t rc = tgp_alloc::dev_malloc(&e->mc, sizeof(TileModelC));
        if (rc != hipSuccess) return fail("hipMalloc", rc);
    }
    if (post) {
        hipError_t rc = grow(&e->rec, &e->rec_cap, (size_t)p.nchunks * (size_t)(p.C + p.Wb) * REC * sizeof(double));
        if (rc != hipSuccess) return fail("hipMalloc", rc);
    }
    if (c.adjoint) {      // (C and Wa are multiples of 8 = kAdjB: plan_tile)
        hipError_t rc = grow(&e->ckpt, &e->ckpt_cap, (size_t)p.nchunks * (size_t)((p.C + p.Wb) / kAdjB) * kAdjState * sizeof(double));
        if (rc == hipSuccess) rc = grow(&e->sums, &e->sums_cap, (size_t)p.nchunks * kAdjSums * sizeof(double));
        if (rc != hipSuccess) return fail("hipMalloc", rc);
    }
    if (draw) {           // (a slot more per chunk: the state the chunk's filter ends on)
        hipError_t rc = grow(&e->ckpt, &e->ckpt_cap, (size_t)p.nchunks * (size_t)((p.C + p.Wb) / kAdjB + 1) * kAdjState * sizeof(double));
        if (rc != hipSuccess) return fail("hipMalloc", rc);
    }
    {      // (the plan's blocks: 9 KB, staged by the runtime before the call returns; the kernel behind it on the same stream reads them)
        hipError_t rc = hipMemcpyAsync(e->mc, &p.mc, sizeof(TileModelC), hipMemcpyHostToDevice, stream);
        if (rc != hipSuccess) return fail("hipMemcpyAsync", rc);
    }
    TArgs ka;
    ka.mc = static_cast<const TileModelC*>(e->mc);
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
    ka.d = p.d;
    ka.mean = c.mean;
    ka.var = c.var;
    ka.rec = static_cast<double*>(e->rec);
    ka.part = e->part;
    ka.gh = c.gh_steps;
    ka.gR = c.gR_steps;
    ka.ckpt = static_cast<double*>(e->ckpt);
    ka.sums = static_cast<double*>(e->sums);
    if (kname) *kname = draw ? draw_kernel_name() : c.adjoint ? adjoint_kernel_name() : kernel_name(post);
    const int xs = (c.R != nullptr ? 1 : 0) | (c.hh != nullptr ? 2 : 0);
    if (draw) {
        DArgs da;
        da.t = ka;
        da.eps_t = c.eps_t;
        da.eps_e = c.eps_e;
        da.y_out = c.y_out;
        for (int k = 0; k < DP; ++k) da.eps_0[k] = k < p.d ? c.eps_0[k] : 0.0;
        switch (xs) {
            case 0: launch_draw<0>(e, stream, da); break;
            case 1: launch_draw<1>(e, stream, da); break;
            case 2: launch_draw<2>(e, stream, da); break;
            default: launch_draw<3>(e, stream, da); break;
        }
    } else if (c.adjoint) {
        switch (xs) {
            case 0: launch_adjoint<0>(e, stream, ka); break;
            case 1: launch_adjoint<1>(e, stream, ka); break;
            case 2: launch_adjoint<2>(e, stream, ka); break;
            default: launch_adjoint<3>(e, stream, ka); break;
        }
    } else {
        switch (xs) {
            case 0: launch_x<0>(e, stream, ka, post); break;
            case 1: launch_x<1>(e, stream, ka, post); break;
            case 2: launch_x<2>(e, stream, ka, post); break;
            default: launch_x<3>(e, stream, ka, post); break;
        }
    }
    hipError_t rc = hipGetLastError();
    if (rc != hipSuccess) return fail("k_sweep_tile launch", rc);
    return 0;
}

void adjoint_blocks(const Engine* e, const tgp_sweep::AdjointOut& o) {
    const int d = e->p.d;
    const double *g = e->part + (size_t)e->p.nchunks * 4, *gv = g + 3 * DP * DP;
    auto block = [d](const double* tile, double* out, bool sym) {      // the d x d corner of a 16 x 16 tile, column-major
        if (!out) return;
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) out[i + j * d] = sym ? 0.5 * (tile[i + DP * j] + tile[j + DP * i]) : tile[i + DP * j];
    };
    block(g, o.gA, false);
    block(g + DP * DP, o.gQ, true);
    block(g + 2 * DP * DP, o.gx0P, true);
    if (o.ga) std::memcpy(o.ga, gv, sizeof(double) * d);
    if (o.gH) std::memcpy(o.gH, gv + DP, sizeof(double) * d);
    if (o.gx0m) std::memcpy(o.gx0m, gv + 2 * DP, sizeof(double) * d);
    if (o.ghh) *o.ghh = gv[3 * DP];
    if (o.gR) *o.gR = gv[3 * DP + 1];
}

double finish(Engine* e, int* status, int* w, int* wb, double* dist_f, double* dist_b) {
    double lml = 0.0, df = 0.0, db = 0.0;
    unsigned bits = 0;
    for (int64_t i = 0; i < e->p.nchunks; ++i) {      // fixed order: the same sum for the same geometry
        const double* q = e->part + (size_t)i * 4;
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

}  // namespace tgp_sweep_tile
