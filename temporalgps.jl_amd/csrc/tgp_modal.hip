// Stationary-gain engine, ONE-LAUNCH path (round 4): logpdf and posterior marginals of an LTI model with one noise variance, scalar
// observations and no missing data in a single kernel over y -- see tgp_modal.hpp.  gfx950 only (wave64, __shfl scans, LDS rows for
// whole-line output stores, uniform coefficients through the kernel-argument segment).
#include "tgp_modal.hpp"
#include "tgp_alloc.hpp"
#include "tgp_lane.hpp"
#include "tgp_lml.hpp"
#include "tgp_post.hpp"
#include "tgp_stream_form.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace tgp_modal {

namespace {

using tgp_plan::HeadTables;
using tgp_plan::Modal;

constexpr int kWJ = 8;      // rows of the WJ / WG tables (a lane of sixteen steps applies them in two halves)
constexpr double kLog2Pi = 1.8378770664093454835606594728112;

// ---- the packed tables of a call (doubles): [0] n1, then the fields at these offsets.  Per-step tables have n0 + 1 rows (row n0: the
// stationary step; the head's steps behind n0 read that row).
struct TabOff {
    int h, mu0, Wm, db, iS, rS, G, c, vb, tvb;
};

// ---- kernel arguments: every coefficient is wave-uniform and reaches the lanes through scalar loads ---------------------------------
template <int D>
struct KArgs {
    double fd[D], fo[D], fb[D], fa[D], fw[D];      // forward:  z' = fd z + fo z_partner + fb u + fa,  r = u - fw . z
    double gd[D], go[D], gc[D], gw[D];             // backward: zeta' = gd zeta + go zeta_partner + gc r,  mean = y - rS r + gw . zeta
    double fpr[6][D], fpi[6][D];                   // M^(SUB 2^k), k < 6 (forward block form: re, signed im; SUB = steps per lane)
    double gpr[6][D], gpi[6][D];
    double ftr[2][D], fti[2][D];                   // M^TILE, M^(2 TILE)
    double gtr[2][D], gti[2][D];
    double WJ[kWJ][D], WG[kWJ][D];
    double hh, rS, vb;
    int n0, nhs, halo, post, rnew_per_step;
    long long T, C, nwg, seq;
    // a time segment of a longer series (one rank of several; single device: wg0 = 0, seg = [0, T), T_eff = T): this launch owns the outputs
    // of [seg_lo, seg_hi) and runs the workgroups wg0 .. wg0 + nwg - 1 of the series; y, mean, var, Rnew (per step) are indexed by the
    // GLOBAL step (the pointers are moved back by seg_lo), the `halo` observations in front of / behind the segment come in yl / yr
    long long wg0, seg_lo, seg_hi, T_eff;
    const double *yl, *yr;
    const double* y;
    const double* Rnew;         // [0]: the shared new noise
    const double* RnewT;        // per-step new noise, indexed by the global step
    double* mean;
    double* var;
    const double* htab;         // pinned host memory: the packed head / tail tables of this call (TabOff), written by the host beside the kernel
    double* tab;                // device memory: workgroup 0 pulls them in here for its head wave
    const long long* flag;      // pinned host memory, one word per stage of the tables: 2 seq (+ 1: declined) once that stage is in `htab`
    TabOff to;
    double* part;               // pinned host memory: [nwg] sum r^2 over the workgroups' core ranges, [nwg] the head's sum r^2 / S
    // The head ON THE HOST (round 5): pinned host memory, flags hold 2 seq once raised.  Workgroup 0 hands the head's nhs observations
    // (and new noise variances) over first thing (hflag[0]), waits -- bounded -- for the head's end state z0 in modal coordinates (hflag[1]) where
    // it used to run the head forwards, hands back the backward state entering the head (zeta_out, hflag[2]) where it used to run it backwards,
    // and a workgroup from the middle of the dispatch writes the head's outputs once the host has them (head_out: nhs means, nhs variances; hflag[3]).
    int hosthead;
    double* head_in;
    const double* z0p;
    double* zeta_out;
    const double* head_out;
    long long* hflag;
};

template <int D>
__device__ __forceinline__ constexpr int partner(int i) {
    return ((i ^ 1) < D) ? (i ^ 1) : i;
}
// x <- P x with P the block form given by (pr, pi): (P x)_i = pr_i x_i + pi_i x_partner(i)
template <int D>
__device__ __forceinline__ void bmul(const double* __restrict__ pr, const double* __restrict__ pi, const double (&x)[D], double (&out)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) out[i] = fma(pr[i], x[i], pi[i] * x[partner<D>(i)]);
}

template <int SUB, int D>
__device__ __forceinline__ void load_lane(const KArgs<D>& ka, long long t0, double (&v)[SUB]) {
    const double* __restrict__ p = ka.y;
    const long long hi = ka.seg_hi < ka.T_eff ? ka.seg_hi : ka.T_eff;
    if (t0 >= ka.seg_lo && t0 + SUB <= hi) {
        if ((reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            const double2* q = reinterpret_cast<const double2*>(p + t0);
#pragma unroll
            for (int j = 0; j < SUB / 2; ++j) {
                const double2 w = q[j];
                v[2 * j] = w.x;
                v[2 * j + 1] = w.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < SUB; ++j) v[j] = p[t0 + j];
        }
    } else {
        // (the ends of the series, and the few lanes of a segment's first / last workgroup that read its neighbours' observations)
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            const long long t = t0 + j;
            double x = 0.0;
            if (t < ka.T_eff) {
                if (t < ka.seg_lo) x = ka.yl[t - (ka.seg_lo - ka.halo)];
                else if (t >= ka.seg_hi) x = ka.yr[t - ka.seg_hi];
                else x = p[t];
            }
            v[j] = x;
        }
    }
}

// A wave's tile of 64 SUB consecutive output values, SUB per lane, leaves through the wave's own LDS row: lane l's SUB / 2 pairs go in at
// 16-byte slots PPL l + l PPL / 16 + j (the pad keeps the 128-bit writes of sixteen lanes on distinct banks) and come out transposed, so that
// every store instruction writes 1 KB of consecutive bytes (as k_apply of tgp_steady.hip).  [lo, hi): the steps this workgroup owns.
// The row holds HALF a tile (the values of 32 lanes: 2 KB + padding); a tile leaves in two rounds -- the LDS a full row would take
// (35 KB per workgroup) cost a workgroup per CU at d = 2, 4 (and would at d = 3 once its registers fit four).
template <int SUB>
struct Row {
    static constexpr int PPL = SUB / 2;                  // pairs per lane
    static constexpr int slots = PPL * 34;               // 16-byte slots of a row: the pairs of 32 lanes, padded
    __device__ static __forceinline__ int lane_slot(int l32) { return PPL * l32 + l32 * PPL / 16; }      // l32: the lane within its half
    __device__ static __forceinline__ int pair_slot(int e) {      // pair e of the half tile (time order)
        const int ls = e / PPL;
        return PPL * ls + ls * PPL / 16 + e % PPL;
    }
};
__device__ __forceinline__ void store_pair(v2d* q, const v2d w) { *q = w; }      // (non-temporal and write-through (sc0 sc1) stores: measured, no difference)
// half_t0: the first step of the half tile in the row
template <int SUB>
__device__ __forceinline__ void flush_row(double* __restrict__ p, long long half_t0, long long lo, long long hi, const v2d* r2, int lane) {
    constexpr int HALF = 32 * SUB;
    const bool aligned = (reinterpret_cast<uintptr_t>(p) & 15) == 0;
    if (half_t0 >= lo && half_t0 + HALF <= hi && aligned) {      // (wave-uniform)
        v2d* q = reinterpret_cast<v2d*>(p + half_t0);
#pragma unroll
        for (int k = 0; k < SUB / 4; ++k) {
            const int e = k * 64 + lane;
            store_pair(q + e, r2[Row<SUB>::pair_slot(e)]);
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < SUB / 4; ++k) {
        const int e = k * 64 + lane;
        const v2d w = r2[Row<SUB>::pair_slot(e)];
        const long long t = half_t0 + 2 * e;
        if (t >= lo && t + 1 < hi && aligned) {
            store_pair(reinterpret_cast<v2d*>(p + t), w);
        } else {
            if (t >= lo && t < hi) p[t] = w.x;
            if (t + 1 >= lo && t + 1 < hi) p[t + 1] = w.y;
        }
    }
}

// ---- the head: steps [0, nhs) with gains of their own, sequentially, by ONE wave.  Nothing in the dependent chain of a step waits for memory:
// the lanes fetch a block's per-step data ahead (lane l the data of step l of the block; the tables are read in place from pinned host memory, so a
// fetch costs a PCIe round trip -- it overlaps the block in work) and a step picks its values out of the lanes' registers with v_readlane.

// one level of the in-row scans: z += (pr, pi) (*) z shifted by OFF lanes inside the row of 16 (DIR 0: from below, 1: from above)
// (level K: OFF = 2^K lanes, the power M^(SUB 2^K) of the kernel arguments -- read member by member: a pointer into the by-value argument
//  struct would make the compiler keep a copy of it in scratch memory)
#define TGP_ROW_LEVEL(DIR, K, PR, PI, Z)                                                                          \
    do {                                                                                                          \
        double g_[D];                                                                                             \
        _Pragma("unroll") for (int i = 0; i < D; ++i) g_[i] = dpp_mov<((DIR) == 0 ? 0x110 : 0x100) + (1 << (K))>(Z[i]); \
        _Pragma("unroll") for (int i = 0; i < D; ++i) Z[i] = fma(ka.PR[K][i], g_[i], fma(ka.PI[K][i], g_[partner<D>(i)], Z[i])); \
    } while (0)

// Forward, in the modal coordinates of the stationary closed loop (O(d) per step; every lane the same arithmetic):
//     z' = M z + fa + fb u + db_t r,   r = u - fw . z,   db_t = V^-1 (A K_t - A K)   (zero from step n0 on)
// Leaves r_t in sR, the end state in z0, sum r^2 / S_t in quad.
template <int D>
__device__ __forceinline__ void head_forward(const KArgs<D>& ka, double* __restrict__ sR /*[kHeadMax]*/, int lane, double (&z0)[D], double& quad) {
    const double* __restrict__ tb = ka.tab;
    const int nhs = ka.nhs, n0 = ka.n0;
    double z[D];
#pragma unroll
    for (int i = 0; i < D; ++i) z[i] = tb[ka.to.mu0 + i];      // (already in modal coordinates: V^-1 (A x0.m + a))
    double acc = 0.0;
    const int nblk = (nhs + 63) >> 6;
    for (int b = 0; b < nblk; ++b) {
        // lane l: the data of step 64 b + l
        const int t = b * 64 + lane, ti = t < n0 ? t : n0;
        const double cy = t < nhs ? ka.y[t] : 0.0, cis = tb[ka.to.iS + ti];
        double cdb[D];
#pragma unroll
        for (int i = 0; i < D; ++i) cdb[i] = tb[ka.to.db + ti * D + i];
        const int cnt = nhs - b * 64 < 64 ? nhs - b * 64 : 64;
        double rk = 0.0;
        for (int s = 0; s < cnt; ++s) {
            const int su = __builtin_amdgcn_readfirstlane(s);
            const double u = readlane_d(cy, su) - ka.hh, is = readlane_d(cis, su);
            double r = u;
#pragma unroll
            for (int i = 0; i < D; ++i) r = fma(-ka.fw[i], z[i], r);
            acc = fma(r * r, is, acc);
            double nz[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double v = fma(ka.fb[i], u, ka.fa[i]);
                v = fma(readlane_d(cdb[i], su), r, v);
                v = fma(ka.fo[i], z[partner<D>(i)], v);
                nz[i] = fma(ka.fd[i], z[i], v);
            }
#pragma unroll
            for (int i = 0; i < D; ++i) z[i] = nz[i];
            rk = (lane == su) ? r : rk;
        }
        if (lane < cnt) sR[b * 64 + lane] = rk;
    }
    lds_sync();
#pragma unroll
    for (int i = 0; i < D; ++i) z0[i] = z[i];
    quad = acc;
}

// Backward over the head from the lam in front of the first stationary step: lam <- G_t lam + c_t r_t (original coordinates: G_t is dense and
// changes per step), mean_t = y_t - (R / S_t) r_t + h . lam.  Lane i < D owns row i of the product; lam goes round by v_readlane.  The rows of
// a chunk of CH steps are staged in LDS (the tables are in device memory by now: a chunk costs an L2 round trip).  sR holds r_t on entry.
template <int D, int CH>
__device__ __forceinline__ void head_backward(const KArgs<D>& ka, const double* __restrict__ sR, double* __restrict__ sTab /*[CH (D D + D)]*/, int lane, const double (&zeta)[D]) {
    constexpr int DD = D * D, ROW = DD + D;
    const double* __restrict__ tb = ka.tab;
    const int nhs = ka.nhs, n0 = ka.n0;
    const int row = lane < D ? lane : D - 1;
    double lam = 0.0, h[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        lam = fma(tb[ka.to.Wm + row * D + k], zeta[k], lam);
        h[k] = tb[ka.to.h + k];
    }
    for (int hi = nhs; hi > 0; hi -= CH) {
        const int lo = hi - CH > 0 ? hi - CH : 0, cnt = hi - lo;
        lds_sync();
        {
            // the chunk's rows [G_t | c_t] are contiguous in the packed tables: 16-byte pieces, four loads in flight per lane and round
            // (a load-store-load chain would cost an L2 round trip per kilobyte; more in flight would cost the kernel's occupancy)
            const v2d* __restrict__ src = reinterpret_cast<const v2d*>(tb + ka.to.G + (size_t)lo * ROW);
            v2d* __restrict__ dst = reinterpret_cast<v2d*>(sTab);
            const int n2 = cnt * ROW / 2;
            for (int base = 0; base < n2; base += 4 * 64) {
                v2d b[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int idx = base + q * 64 + lane;
                    b[q] = src[idx < n2 ? idx : n2 - 1];
                }
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int idx = base + q * 64 + lane;
                    if (idx < n2) dst[idx] = b[q];
                }
            }
        }
        const int t = lo + lane, ti = t < n0 ? t : n0;
        const double cy = (lane < cnt) ? ka.y[t] : 0.0, crs = tb[ka.to.rS + ti], cr = (lane < cnt) ? sR[t] : 0.0;
        lds_sync();
        double mk = 0.0;
        // the row of the first step to be processed (the chunk's last)
        double g[D], cc;
        {
            const double* __restrict__ rw = sTab + (cnt - 1) * ROW;
#pragma unroll
            for (int k = 0; k < D; ++k) g[k] = rw[row * D + k];
            cc = rw[DD + row];
        }
        for (int s = cnt - 1; s >= 0; --s) {
            const int su = __builtin_amdgcn_readfirstlane(s);
            double gn[D], cn = 0.0;                  // the next step's row, in flight while this one's chain runs
            {
                const double* __restrict__ rw = sTab + (su > 0 ? su - 1 : 0) * ROW;
#pragma unroll
                for (int k = 0; k < D; ++k) gn[k] = rw[row * D + k];
                cn = rw[DD + row];
            }
            const double r = readlane_d(cr, su), yv = readlane_d(cy, su), rs = readlane_d(crs, su);
            double m = fma(-rs, r, yv), nl = cc * r;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double lk = readlane_d(lam, k);
                m = fma(h[k], lk, m);
                nl = fma(g[k], lk, nl);
            }
            lam = nl;
            mk = (lane == su) ? m : mk;
#pragma unroll
            for (int k = 0; k < D; ++k) g[k] = gn[k];
            cc = cn;
        }
        if (lane < cnt) ka.mean[t] = mk;
    }
}

// ---- the head by SCANS over its steps (d <= 4): a tile of 64 head steps at a time, lane t the affine map of step t -- (P_t, c_t) with
// P_t = M - db_t fw', c_t = (fb + db_t) u_t + fa forwards, (G_t, c_t r_t) backwards -- composed over the lanes in six levels of DPP moves
// (rows of 16 by row_shr / row_shl, then across the rows), d^2 + d values moved and d^3 + d^2 FMAs per level: ~400 instructions per
// 64 steps at d = 3 where the sequential form above spends 64 x 40 and a 64-step dependent chain (12.8 us against ~2).  From d = 5
// on an element no longer fits the registers the tiles' code leaves (3 (d^2 + d) doubles): those heads stay sequential.
// new <- mine o neighbour:  P <- P Pn,  c <- P cn + c   (row by row: a row of P is replaced once it has been used)
template <int D>
__device__ __forceinline__ void compose_after(double (&P)[D][D], double (&c)[D], const double (&Pn)[D][D], const double (&cn)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double row[D], ci = c[i];
#pragma unroll
        for (int k = 0; k < D; ++k) row[k] = 0.0;
#pragma unroll
        for (int m = 0; m < D; ++m) {
            ci = fma(P[i][m], cn[m], ci);
#pragma unroll
            for (int k = 0; k < D; ++k) row[k] = fma(P[i][m], Pn[m][k], row[k]);
        }
#pragma unroll
        for (int k = 0; k < D; ++k) P[i][k] = row[k];
        c[i] = ci;
    }
}
// the neighbour's element by one DPP control (lanes without a source, rows outside the mask: the identity), composed into mine
template <int D, int CTRL, int ROWMASK>
__device__ __forceinline__ void scan_level(double (&P)[D][D], double (&c)[D], bool has) {
    double Pn[D][D], cn[D];
    const double one = has ? 0.0 : 1.0;
#pragma unroll
    for (int i = 0; i < D; ++i) {
        cn[i] = dpp_mov<CTRL, ROWMASK>(c[i]);
#pragma unroll
        for (int k = 0; k < D; ++k) Pn[i][k] = dpp_mov<CTRL, ROWMASK>(P[i][k]) + (i == k ? one : 0.0);
    }
    compose_after<D>(P, c, Pn, cn);
}

template <int D>
__device__ __forceinline__ void head_forward_scan(const KArgs<D>& ka, double* __restrict__ sR /*[kHeadMax]*/, int lane, double (&z0out)[D], double& quad) {
    const double* __restrict__ tb = ka.tab;
    const int nhs = ka.nhs, n0 = ka.n0;
    double z0[D];
#pragma unroll
    for (int i = 0; i < D; ++i) z0[i] = tb[ka.to.mu0 + i];      // (already in modal coordinates: V^-1 (A x0.m + a))
    double acc = 0.0;
    for (int t0 = 0; t0 < nhs; t0 += 64) {
        const int cnt = nhs - t0 < 64 ? nhs - t0 : 64;
        const bool valid = lane < cnt;
        const int t = valid ? t0 + lane : t0, ti = t < n0 ? t : n0;
        const double u = ka.y[t] - ka.hh, is = tb[ka.to.iS + ti];
        double P[D][D], c[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double db = tb[ka.to.db + ti * D + i];
            c[i] = valid ? fma(ka.fb[i] + db, u, ka.fa[i]) : 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const double m = (k == i) ? ka.fd[i] : ((k == partner<D>(i)) ? ka.fo[i] : 0.0);
                P[i][k] = valid ? fma(-db, ka.fw[k], m) : (i == k ? 1.0 : 0.0);
            }
        }
        const int p = lane & 15;
        scan_level<D, 0x111, 0xF>(P, c, p >= 1);
        scan_level<D, 0x112, 0xF>(P, c, p >= 2);
        scan_level<D, 0x114, 0xF>(P, c, p >= 4);
        scan_level<D, 0x118, 0xF>(P, c, p >= 8);
        scan_level<D, 0x142, 0xA>(P, c, (lane & 16) != 0);      // rows 1, 3: everything up to the end of the row below
        scan_level<D, 0x143, 0xC>(P, c, lane >= 32);            // rows 2, 3: everything up to lane 31
        // the state behind step t, in front of it (the left neighbour's; lane 0: the tile's start state), the innovation
        double za[D], r = u;
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double v = c[i];
#pragma unroll
            for (int k = 0; k < D; ++k) v = fma(P[i][k], z0[k], v);
            za[i] = v;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double sh = dpp_mov<0x138>(za[i]);
            r = fma(-ka.fw[i], lane == 0 ? z0[i] : sh, r);
        }
        if (valid) {
            acc = fma(r * r, is, acc);
            sR[t0 + lane] = r;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) z0[i] = readlane_d(za[i], cnt - 1);
    }
    lds_sync();
#pragma unroll
    for (int i = 0; i < D; ++i) z0out[i] = z0[i];
    quad = readlane_d(wave_sum_to_lane63(acc), 63);
}

template <int D>
__device__ __forceinline__ void head_backward_scan(const KArgs<D>& ka, const double* __restrict__ sR, int lane, const double (&zeta)[D]) {
    constexpr int DD = D * D, ROW = DD + D;
    const double* __restrict__ tb = ka.tab;
    const int nhs = ka.nhs, n0 = ka.n0;
    double lamR[D], h[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < D; ++k) v = fma(tb[ka.to.Wm + i * D + k], zeta[k], v);
        lamR[i] = v;
        h[i] = tb[ka.to.h + i];
    }
    for (int t0 = ((nhs - 1) >> 6) << 6; t0 >= 0; t0 -= 64) {
        const int cnt = nhs - t0 < 64 ? nhs - t0 : 64;
        const bool valid = lane < cnt;
        const int t = valid ? t0 + lane : t0, ti = t < n0 ? t : n0;
        const double yt = ka.y[t], rs = tb[ka.to.rS + ti], r = sR[t];
        const double* __restrict__ rw = tb + ka.to.G + (size_t)t * ROW;      // [G_t | c_t], one row of the packed tables per head step
        double P[D][D], c[D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            c[i] = valid ? rw[DD + i] * r : 0.0;
#pragma unroll
            for (int k = 0; k < D; ++k) P[i][k] = valid ? rw[i * D + k] : (i == k ? 1.0 : 0.0);
        }
        // suffix scan: lane t <- the steps t .. end of the tile (the neighbour holds the LATER steps, applied first)
        const int p = lane & 15;
        scan_level<D, 0x101, 0xF>(P, c, p + 1 < 16);
        scan_level<D, 0x102, 0xF>(P, c, p + 2 < 16);
        scan_level<D, 0x104, 0xF>(P, c, p + 4 < 16);
        scan_level<D, 0x108, 0xF>(P, c, p + 8 < 16);
        {
            // rows 0 and 2 take the first lane of the row above them: wave_shl:1 brings it to their lane 15, row_newbcast:15 spreads it
            double Pn[D][D], cn[D];
            const double one = (lane & 16) == 0 ? 0.0 : 1.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                cn[i] = dpp_mov<0x15F, 0x5>(dpp_mov<0x130>(c[i]));
#pragma unroll
                for (int k = 0; k < D; ++k) Pn[i][k] = dpp_mov<0x15F, 0x5>(dpp_mov<0x130>(P[i][k])) + (i == k ? one : 0.0);
            }
            compose_after<D>(P, c, Pn, cn);
            // the lower half takes lane 32 (complete by now)
            const bool lower = lane < 32;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double x = readlane_d(c[i], 32);
                cn[i] = lower ? x : 0.0;
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const double v = readlane_d(P[i][k], 32);
                    Pn[i][k] = lower ? v : (i == k ? 1.0 : 0.0);
                }
            }
            compose_after<D>(P, c, Pn, cn);
        }
        // lam behind step t (what the steps t .. end make of the tile's right-hand input); in front of it: the right neighbour's
        double lo[D], m = fma(-rs, r, yt);
#pragma unroll
        for (int i = 0; i < D; ++i) {
            double v = c[i];
#pragma unroll
            for (int k = 0; k < D; ++k) v = fma(P[i][k], lamR[k], v);
            lo[i] = v;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            const double sh = dpp_mov<0x130>(lo[i]);
            m = fma(h[i], lane == 63 ? lamR[i] : sh, m);
        }
        if (valid) ka.mean[t0 + lane] = m;
#pragma unroll
        for (int i = 0; i < D; ++i) lamR[i] = readlane_d(lo[i], 0);
    }
}

// The head's variances: data-independent, the last stage of the tables (read in place from pinned memory: at most kHeadMax values)
template <int D>
__device__ __forceinline__ void head_variances(const KArgs<D>& ka, int lane) {
    wait_tables(ka.flag + 2, ka.seq);
    const double rn0 = ka.Rnew[0];
    const double* __restrict__ vb = ka.htab + ka.to.vb;
    for (int t = lane; t < ka.nhs; t += 64) ka.var[t] = vb[t < ka.n0 ? t : ka.n0] + (ka.rnew_per_step ? ka.RnewT[t] : rn0);
}

// =================================================================================================================================
// The kernel.  Workgroup g owns the steps [nhs + g C, nhs + (g + 1) C) (its core); its NW waves are NW consecutive tiles of 64 SUB steps
// that start `halo` steps earlier (g = 0: at nhs, with the head's exact end state) and end `halo` steps later.  Both mean recursions have
// forgotten a state after `halo` steps (tgp_steady_plan.hpp: |eigenvalue|^halo <= 2^-64), so a zero state at the start of the span and
// a zero lam at its end give every core step the same values, to rounding, as the recursion over the whole series: no pass over y
// before this one, no carries between workgroups.  Inside the workgroup the tiles are chained exactly (through LDS, over the at most
// three preceding / following tiles -- whatever lies further back has decayed as well).
// A lane holds SUB consecutive steps: 8, or 16 (the in-tile scans cost the same per level whatever a lane holds, so sixteen halve them
// per step -- at the price of 32 more registers).
// =================================================================================================================================
// The per-lane power table sPw[dir][re / im][component][lane]: job (dir, i) is one chain of 6 conditional complex multiplications by the bits of
// the lane's exponent; wave JOB mod NW runs it.  Direction and component are compile-time constants: every coefficient is a scalar load from
// the kernel arguments (a run-time index into the by-value argument struct would make the compiler keep a copy of it in scratch memory)
template <int D, int NW, int JOB>
struct PowerJobs {
    __device__ static __forceinline__ void run(const KArgs<D>& ka, double (*sPw)[2][D][64], int lane, int uw) {
        if constexpr (JOB < 2 * D) {
            if (uw == JOB % NW) {      // (wave-uniform)
                constexpr int dir = JOB / D, i = JOB % D;      // direction (0: forward, 1: backward), component
                const int e = dir == 0 ? lane : 63 - lane;
                double xr = 1.0, xi = 0.0;                      // the block form of M^(SUB e): (re, signed im) of the component, from the identity
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const double pr = dir == 0 ? ka.fpr[k][i] : ka.gpr[k][i], pi = dir == 0 ? ka.fpi[k][i] : ka.gpi[k][i];
                    const bool bit = ((e >> k) & 1) != 0;
                    // (a + i b)(c + i d) with the signed-imaginary convention: re = a c - b d, im = a d + b c (the sign of the pair's second member follows)
                    const double nr = fma(xr, pr, -(xi * pi)), ni = fma(xr, pi, xi * pr);
                    xr = bit ? nr : xr;
                    xi = bit ? ni : xi;
                }
                sPw[dir][0][i][lane] = xr;
                sPw[dir][1][i][lane] = xi;
            }
            PowerJobs<D, NW, JOB + 1>::run(ka, sPw, lane, uw);
        }
    }
};

// Development build (-DTGP_MODAL_PROBE): wave 0 of a mid-series workgroup stamps its phases (shader clock) into part[nwg + 12 ..]
#ifdef TGP_MODAL_PROBE
#define TGP_STAMP(k)                                                                     \
    do {                                                                                 \
        __builtin_amdgcn_sched_barrier(0);                                               \
        if (probe_wave) {                                                                \
            const double now = (double)clock64();                                        \
            if (lane == 0) ka.part[ka.nwg + 12 + (k)] = now;                             \
        }                                                                                \
        __builtin_amdgcn_sched_barrier(0);                                               \
    } while (0)
#else
#define TGP_STAMP(k) do { } while (0)
#endif
// waves per SIMD the register allocation is held to (a workgroup of 8 waves puts two on each SIMD): d <= 2 fit four workgroups per CU as they
// are (64 registers), d = 3, 4 are held to three; beyond, what the code needs (d = 5 would spill at 80).  Measured with the half rows that
// freed the LDS for it: a fourth workgroup at d = 2 and a third at d = 4 change nothing -- in its steady state the kernel moves ~6 TB/s,
// what a copy reaches; its time at T = 1e7 is that plus the ramps at both ends
#define TGP_MIN_WAVES(D, NW, HS) ((NW) == 8 ? ((HS) ? 4 : (((D) == 3 || (D) == 4) ? 6 : 4)) : 2)
template <int D, int NW, int SUB, bool HEAD_SCANS>
__global__ __launch_bounds__(NW * 64, TGP_MIN_WAVES(D, NW, HEAD_SCANS)) void k_steady_one(const KArgs<D> ka_by_value) {
    // The arguments are read where they lie, in the kernel-argument segment (scalar loads, any index): a by-value struct is first copied to a
    // private variable, and one access pattern the optimiser cannot take apart (a run-time index, or identical blocks it merges into one
    // with the offsets in a phi) leaves the whole 3 KB struct in scratch memory -- 20 x the kernel's time, from one build to the next
    (void)ka_by_value;
    const KArgs<D>& ka = *(const KArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();      // (an address-space cast: C style)
    static_assert(SUB == kWJ, "eight steps per lane (sixteen were built and measured in round 4: the 32 more registers cost more occupancy than the halved scans save)");
    constexpr int TILE = 64 * SUB;
    constexpr int CHB = D <= 4 ? 64 : (D <= 6 ? 32 : 16);      // steps of the head's backward recursion staged in LDS at a time (~10 KB)
    __shared__ double sF[NW][D], sB[NW][D], sHead[D], sAcc[NW];
    __shared__ double sR[tgp_plan::kHeadMax];
    __shared__ __attribute__((aligned(16))) double sTab[(HEAD_SCANS && D <= 4) ? 2 : CHB * (D * D + D)];      // (the head as scans: nothing staged)
    __shared__ __attribute__((aligned(16))) double sOut[NW][2 * Row<SUB>::slots];
    // M^(SUB l) (forward) and Mg^(SUB (63 - l)) (backward) for the lanes l of a tile: what carries a tile's start state / right-hand input to
    // its lanes.  The same for every wave: the waves share the building (by the bits of the lane number) between them
    __shared__ double sPw[2][2][D][64];
    __shared__ double sPoison;      // NaN once a bounded wait for the host ran out (host head): the call's result is then discarded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) sPoison = 0.0;
    // XCD-aware order: consecutive workgroups (which share their halos' lines of y) land on the same XCD, hence the same L2
    long long wg;
    {
        const long long per = (ka.nwg + 7) / 8;
        wg = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
        if ((long long)(blockIdx.x >> 3) >= per || wg >= ka.nwg) return;
    }
    const long long T = ka.T, Tv = ka.T_eff;      // Tv: the steps this launch may read (a segment: its own and `halo` beyond)
    const long long g = ka.wg0 + wg;               // the workgroup's number in the series
    long long c_lo = ka.nhs + g * ka.C, c_hi_raw = c_lo + ka.C;
    c_lo = c_lo > ka.seg_lo ? c_lo : ka.seg_lo;
    c_hi_raw = c_hi_raw < ka.seg_hi ? c_hi_raw : ka.seg_hi;
    const long long c_hi = c_hi_raw < T ? c_hi_raw : T;
    const bool first = g == 0 && ka.seg_lo == 0;      // the workgroup behind the head (a later segment may begin inside the series' first core range)
    const long long s0 = first ? (long long)ka.nhs : c_lo - ka.halo;
    const long long tile_t0 = s0 + (long long)wave * TILE, t0 = tile_t0 + (long long)lane * SUB;
    const bool head_wave = first && wave == 0;
    const bool any_valid = tile_t0 < Tv;                             // (wave-uniform)
    const bool need_back = any_valid && tile_t0 + TILE > c_lo;       // a tile wholly inside the left halo only hands its end state on
    const bool has_out = ka.post && need_back && tile_t0 < c_hi;

    const bool probe_wave = wg == (ka.nwg >> 1) && wave == 0;
    (void)probe_wave;
    const bool probe = wg == (ka.nwg >> 1) && threadIdx.x == 0;      // (TGP_STEADY_DEBUG: a mid-series workgroup's lifetime in shader cycles and in 100 MHz ticks)
    if (probe) {
        ka.part[ka.nwg + 8] = (double)clock64();
        ka.part[ka.nwg + 9] = (double)wall_clock64();
    }
    double head_quad = 0.0;
    if (first && ka.hosthead) {
        if (wave == NW - 1) {      // the head's inputs to the host, first thing: its forward recursion runs there
            for (int t = lane; t < ka.nhs; t += 64) {
                ka.head_in[t] = ka.y[t];
                if (ka.post && ka.rnew_per_step) ka.head_in[ka.nhs + t] = ka.RnewT[t];
            }
            if (ka.post && !ka.rnew_per_step && lane == 0) ka.head_in[ka.nhs] = ka.Rnew[0];
            __threadfence_system();
            if (lane == 0) __hip_atomic_store(ka.hflag, 2 * ka.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    } else if (first) {
        // the head's tables: wait for the host, pull them into device memory (all waves), then the head wave runs the head forward
        if (threadIdx.x == 0) ka.part[ka.nwg + 1] = (double)wall_clock64();      // (phases of workgroup 0, 100 MHz: TGP_STEADY_DEBUG prints them)
        wait_tables(ka.flag, ka.seq, threadIdx.x == 0 ? &ka.part[ka.nwg] : nullptr);      // (timed out: the head's share becomes NaN)
        if (threadIdx.x == 0) ka.part[ka.nwg + 2] = (double)wall_clock64();
        const v2d* __restrict__ src = reinterpret_cast<const v2d*>(ka.htab);
        v2d* __restrict__ dst = reinterpret_cast<v2d*>(ka.tab);
        for (int idx = threadIdx.x; idx < ka.to.G / 2; idx += NW * 64) dst[idx] = src[idx];      // (stage 0: everything in front of the rows [G_t | c_t])
        __syncthreads();
        if (head_wave) {
            double z0[D];
            __builtin_amdgcn_s_setprio(3);      // (the one sequential wave of the launch: ahead of the tiles' waves it shares its SIMD with)
            if constexpr (HEAD_SCANS && D <= 4) head_forward_scan<D>(ka, sR, lane, z0, head_quad);
            else head_forward<D>(ka, sR, lane, z0, head_quad);
            __builtin_amdgcn_s_setprio(0);
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < D; ++i) sHead[i] = z0[i];
                ka.part[ka.nwg + 3] = (double)wall_clock64();
            }
        } else if (ka.post) {
            // meanwhile the other waves fetch stage 1, the rows of the head's backward recursion (the barrier below hands them to the head wave)
            wait_tables(ka.flag + 1, ka.seq);
            for (int idx = ka.to.G / 2 + (int)threadIdx.x - 64; idx < ka.to.vb / 2; idx += (NW - 1) * 64) dst[idx] = src[idx];
        }
    }
    // ---- forward, zero start: innovations r0 of the lane's steps, the lane's end state, inclusive scan over the lanes
    double yv[SUB], r[SUB], st[D];
    const long long left = Tv - t0;
    const int nvalid = left >= SUB ? SUB : (left > 0 ? (int)left : 0);
    // (2 D chains of 6 conditional complex multiplications -- shared out over the waves, one component of one direction each, while the
    //  observations are on their way; two waves doing all of it made the other six wait at the barrier: 9 000 cycles at d = 6)
    auto build_powers = [&]() { PowerJobs<D, NW, 0>::run(ka, sPw, lane, __builtin_amdgcn_readfirstlane(wave)); };
    TGP_STAMP(0);
    if (any_valid) load_lane<SUB, D>(ka, t0, yv);
    // (the new noise is wanted at the very end, by the variance stores: fetched here, beside the observations, not in front of those stores)
    const double rn0 = (ka.post && !ka.rnew_per_step) ? ka.Rnew[0] : 0.0;
    build_powers();
    __syncthreads();      // (the in-tile scans below read the table; the observations are still on their way)
    {
        double z[D];
#pragma unroll
        for (int i = 0; i < D; ++i) z[i] = 0.0;
        if (any_valid) {
#ifdef TGP_MODAL_PROBE
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
            TGP_STAMP(1);
#pragma unroll
            for (int j = 0; j < SUB; ++j) {
                const double u = yv[j] - ka.hh;
                double rr = u;
#pragma unroll
                for (int i = 0; i < D; ++i) rr = fma(-ka.fw[i], z[i], rr);
                r[j] = rr;
                double nz[D];
#pragma unroll
                for (int i = 0; i < D; ++i) nz[i] = fma(ka.fd[i], z[i], fma(ka.fo[i], z[partner<D>(i)], fma(ka.fb[i], u, ka.fa[i])));
#pragma unroll
                for (int i = 0; i < D; ++i) z[i] = nz[i];
            }
            TGP_STAMP(2);
            // inclusive scan over the lanes without an LDS round trip: four levels inside the rows of 16 lanes (row_shr moves), then the rows'
            // end states across (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) through the per-lane powers of the table
            TGP_ROW_LEVEL(0, 0, fpr, fpi, z);
            TGP_ROW_LEVEL(0, 1, fpr, fpi, z);
            TGP_ROW_LEVEL(0, 2, fpr, fpi, z);
            TGP_ROW_LEVEL(0, 3, fpr, fpi, z);
            {
                const int e1 = (lane & 15) + 1;                 // lane 16 r + p takes M^(SUB (p + 1)) times the state behind lane 16 r - 1
                double g[D];
#pragma unroll
                for (int i = 0; i < D; ++i) g[i] = dpp_mov<0x142, 0xA>(z[i]);
#pragma unroll
                for (int i = 0; i < D; ++i) z[i] = fma(sPw[0][0][i][e1], g[i], fma(sPw[0][1][i][e1], g[partner<D>(i)], z[i]));
                const int e2 = lane >= 32 ? lane - 31 : 0;      // lane l >= 32 takes M^(SUB (l - 31)) times the state behind lane 31
#pragma unroll
                for (int i = 0; i < D; ++i) g[i] = dpp_mov<0x143, 0xC>(z[i]);
#pragma unroll
                for (int i = 0; i < D; ++i) z[i] = fma(sPw[0][0][i][e2], g[i], fma(sPw[0][1][i][e2], g[partner<D>(i)], z[i]));
            }
        }
#pragma unroll
        for (int i = 0; i < D; ++i) st[i] = dpp_mov<0x138>(z[i]);      // the state in front of the lane's steps: its left neighbour's (lane 0: zero)
        if (lane == 63) {
#pragma unroll
            for (int i = 0; i < D; ++i) sF[wave][i] = any_valid ? z[i] : 0.0;
        }
    }
    TGP_STAMP(3);
#ifdef TGP_MODAL_PROBE
    if (wg == (ka.nwg >> 1) && lane == 0) ka.part[ka.nwg + 28 + wave] = (double)clock64();      // every wave's arrival at barrier 1 ...
#endif
    __syncthreads();
    TGP_STAMP(4);
    double acc = 0.0;
    double zst[D];
#pragma unroll
    for (int i = 0; i < D; ++i) zst[i] = 0.0;
    if (any_valid) {
        // the tile's start state from the (at most three) tiles before it; workgroup 0: the head's end state sits at position -1
        double zin[D];
#pragma unroll
        for (int i = 0; i < D; ++i) zin[i] = 0.0;
        if (first && ka.hosthead && wave < 3) wait_tables(ka.hflag + 1, ka.seq, &sPoison);      // (wave-uniform) the head's end state comes from the host: z0p below
#pragma unroll
        for (int k = 1; k <= 3; ++k) {
            const int src = wave - k;
            if (src < -1 || (src == -1 && !first)) continue;      // (wave-uniform)
            double x[D];
#pragma unroll
            for (int i = 0; i < D; ++i) x[i] = (src >= 0) ? sF[src][i] : (ka.hosthead ? ka.z0p[i] : sHead[i]);
            if (k == 1) {
#pragma unroll
                for (int i = 0; i < D; ++i) zin[i] += x[i];
            } else {
                double px[D];
                bmul<D>(ka.ftr[k - 2], ka.fti[k - 2], x, px);
#pragma unroll
                for (int i = 0; i < D; ++i) zin[i] += px[i];
            }
        }
        // the lane's start state: st + M^(SUB lane) zin
#pragma unroll
        for (int i = 0; i < D; ++i) st[i] = fma(sPw[0][0][i][lane], zin[i], fma(sPw[0][1][i][lane], zin[partner<D>(i)], st[i]));
        const bool in_core = t0 >= c_lo && t0 < c_hi_raw;
        // the start state moves step j's innovation by -fw' M^j st
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            double rr = r[j];
#pragma unroll
            for (int i = 0; i < D; ++i) rr = fma(-ka.WJ[j][i], st[i], rr);
            rr = (j < nvalid) ? rr : 0.0;
            r[j] = rr;
            acc = fma(rr, rr, acc);
        }
        acc = in_core ? acc : 0.0;
    }
    if (!ka.post) {
        // logpdf only: the sum of squares is all that is wanted
        acc = wave_sum_to_lane63(acc);
        if (lane == 63) sAcc[wave] = acc;
        __syncthreads();
        if (threadIdx.x == 0) {
            double t = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) t += sAcc[w];
            ka.part[wg] = t + sPoison;
            if (first) ka.part[ka.nwg] = head_quad;
        }
        return;
    }
    // ---- backward, zero lam behind the tile: m0_j = y_j - rS r_j + gw . zeta (zeta from the lane's own later steps), reverse scan
    TGP_STAMP(5);
    if (need_back) {
        double zeta[D];
#pragma unroll
        for (int i = 0; i < D; ++i) zeta[i] = 0.0;
#pragma unroll
        for (int j = SUB - 1; j >= 0; --j) {
            double m = fma(-ka.rS, r[j], yv[j]);
#pragma unroll
            for (int i = 0; i < D; ++i) m = fma(ka.gw[i], zeta[i], m);
            yv[j] = m;
            double nz[D];
#pragma unroll
            for (int i = 0; i < D; ++i) nz[i] = fma(ka.gd[i], zeta[i], fma(ka.go[i], zeta[partner<D>(i)], ka.gc[i] * r[j]));
#pragma unroll
            for (int i = 0; i < D; ++i) zeta[i] = nz[i];
        }
        TGP_STAMP(6);
        // the reverse scan: rows by row_shl moves; then rows 0 and 2 take the first lane of the row above them (wave_shl:1 brings it to their
        // lane 15, row_newbcast:15 spreads it), then the lower half takes lane 32 (a scalar by v_readlane)
        TGP_ROW_LEVEL(1, 0, gpr, gpi, zeta);
        TGP_ROW_LEVEL(1, 1, gpr, gpi, zeta);
        TGP_ROW_LEVEL(1, 2, gpr, gpi, zeta);
        TGP_ROW_LEVEL(1, 3, gpr, gpi, zeta);
        {
            const int e1 = 47 + (lane & 15);                  // Mg^(SUB (16 - p)) sits at position 63 - (16 - p) of the backward table
            double g[D];
#pragma unroll
            for (int i = 0; i < D; ++i) g[i] = dpp_mov<0x15F, 0x5>(dpp_mov<0x130>(zeta[i]));
#pragma unroll
            for (int i = 0; i < D; ++i) zeta[i] = fma(sPw[1][0][i][e1], g[i], fma(sPw[1][1][i][e1], g[partner<D>(i)], zeta[i]));
            const int e2 = lane < 32 ? 31 + lane : 63;        // Mg^(SUB (32 - l)) at position 63 - (32 - l); the upper half: the identity's place, times zero
            const double keep = lane < 32 ? 1.0 : 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) g[i] = readlane_d(zeta[i], 32) * keep;
#pragma unroll
            for (int i = 0; i < D; ++i) zeta[i] = fma(sPw[1][0][i][e2], g[i], fma(sPw[1][1][i][e2], g[partner<D>(i)], zeta[i]));
        }
#pragma unroll
        for (int i = 0; i < D; ++i) zst[i] = dpp_mov<0x130>(zeta[i]);      // the lam behind the lane's steps: its right neighbour's (lane 63: zero)
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < D; ++i) sB[wave][i] = zeta[i];
        }
    } else if (lane == 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) sB[wave][i] = 0.0;
    }
    TGP_STAMP(7);
#ifdef TGP_MODAL_PROBE
    if (wg == (ka.nwg >> 1) && lane == 0) ka.part[ka.nwg + 28 + NW + wave] = (double)clock64();      // ... and at barrier 2
#endif
    __syncthreads();
    TGP_STAMP(8);
    // the lam entering a tile from the right: from the (at most three) tiles behind it
    auto right_input = [&](int w, double (&zin)[D]) {
#pragma unroll
        for (int i = 0; i < D; ++i) zin[i] = 0.0;
#pragma unroll
        for (int k = 1; k <= 3; ++k) {
            const int src = w + k;
            if (src >= NW) continue;
            double x[D];
#pragma unroll
            for (int i = 0; i < D; ++i) x[i] = sB[src][i];
            if (k == 1) {
#pragma unroll
                for (int i = 0; i < D; ++i) zin[i] += x[i];
            } else {
                double px[D];
                bmul<D>(ka.gtr[k - 2], ka.gti[k - 2], x, px);
#pragma unroll
                for (int i = 0; i < D; ++i) zin[i] += px[i];
            }
        }
    };
    if (has_out) {
        double zin[D];
        right_input(wave, zin);
#pragma unroll
        for (int i = 0; i < D; ++i) zst[i] = fma(sPw[1][0][i][lane], zin[i], fma(sPw[1][1][i][lane], zin[partner<D>(i)], zst[i]));
        v2d* row = reinterpret_cast<v2d*>(sOut[wave]);
        const int wb = Row<SUB>::lane_slot(lane & 31);
        // the lam behind the lane's last step reaches step j through Mg^(SUB - 1 - j): WG holds gw' Mg^(7 - j)
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            double m = yv[j];
#pragma unroll
            for (int i = 0; i < D; ++i) m = fma(ka.WG[j][i], zst[i], m);
            yv[j] = m;
        }
        TGP_STAMP(9);
        // out through the wave's LDS row, half a tile at a time (the lower 32 lanes' values, then the upper 32's)
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            if ((lane >> 5) == half) {
#pragma unroll
                for (int j = 0; j < SUB; j += 2) {
                    v2d w;
                    w.x = yv[j];
                    w.y = yv[j + 1];
                    row[wb + (j >> 1)] = w;
                }
            }
            lds_sync();
            flush_row<SUB>(ka.mean, tile_t0 + half * (TILE / 2), c_lo, c_hi, row, lane);
            lds_sync();
        }
        TGP_STAMP(10);
        // the variances do not depend on the data: a constant outside the last n1 steps (plus the new noise); written transposed as well
        {
            long long n1 = 0;
            if (T - tile_t0 <= (long long)tgp_plan::kTailMax + TILE) {      // (wave-uniform: the last few tiles of the series)
                wait_tables(ka.flag + 2, ka.seq);
                n1 = (long long)ka.htab[0];
            }
            const double* __restrict__ tvb = ka.htab + ka.to.tvb;      // (in place from pinned memory: the last few tiles, a handful of values)
            const bool aligned = (reinterpret_cast<uintptr_t>(ka.var) & 15) == 0 && (!ka.rnew_per_step || (reinterpret_cast<uintptr_t>(ka.RnewT) & 15) == 0);
            // (wave-uniform: a tile inside the workgroup's range, away from the series' end, one shared new noise -- nearly every tile: one constant)
            const bool plain = aligned && !ka.rnew_per_step && n1 == 0 && tile_t0 >= c_lo && tile_t0 + TILE <= c_hi;
            if (plain) {
                v2d w;
                w.x = ka.vb + rn0;
                w.y = w.x;
                v2d* q = reinterpret_cast<v2d*>(ka.var + tile_t0);
#pragma unroll
                for (int k = 0; k < SUB / 2; ++k) store_pair(q + k * 64 + lane, w);
            } else
#pragma unroll
            for (int k = 0; k < SUB / 2; ++k) {
                const long long t = tile_t0 + 2 * (k * 64 + lane);
                if (t + 1 < c_lo || t >= c_hi) continue;
                double v0 = ka.vb, v1 = ka.vb;
                const long long b0 = T - 1 - t, b1 = b0 - 1;
                if (b0 < n1) {                           // (the last tiles only)
                    if (b0 >= 0) v0 = tvb[b0];
                    if (b1 >= 0) v1 = tvb[b1];
                } else if (b1 < n1 && b1 >= 0) {
                    v1 = tvb[b1];
                }
                if (t >= c_lo && t + 1 < c_hi && aligned) {
                    v2d rn;
                    if (ka.rnew_per_step) {
                        rn = *reinterpret_cast<const v2d*>(ka.RnewT + t);
                    } else {
                        rn.x = rn0;
                        rn.y = rn0;
                    }
                    v2d w;
                    w.x = v0 + rn.x;
                    w.y = v1 + rn.y;
                    store_pair(reinterpret_cast<v2d*>(ka.var + t), w);
                } else {
                    if (t >= c_lo && t < c_hi) ka.var[t] = v0 + (ka.rnew_per_step ? ka.RnewT[t] : rn0);
                    if (t + 1 >= c_lo && t + 1 < c_hi) ka.var[t + 1] = v1 + (ka.rnew_per_step ? ka.RnewT[t + 1] : rn0);
                }
            }
        }
    }
    TGP_STAMP(11);
    if (head_wave && ka.hosthead) {
        double zin[D];
        right_input(-1, zin);
        if (lane == 0) {      // the backward state entering the head: the host runs the head backwards from it
#pragma unroll
            for (int i = 0; i < D; ++i) ka.zeta_out[i] = zin[i];
            __threadfence_system();
            __hip_atomic_store(ka.hflag + 2, 2 * ka.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    } else if (head_wave) {
        double zin[D];
        right_input(-1, zin);
        if (lane == 0) ka.part[ka.nwg + 4] = (double)wall_clock64();
        __builtin_amdgcn_s_setprio(3);
        if constexpr (HEAD_SCANS && D <= 4) head_backward_scan<D>(ka, sR, lane, zin);
        else head_backward<D, CHB>(ka, sR, sTab, lane, zin);
        __builtin_amdgcn_s_setprio(0);
        if (lane == 0) ka.part[ka.nwg + 5] = (double)wall_clock64();
        head_variances<D>(ka, lane);
    }
    // the head's outputs come from the host: a workgroup from the MIDDLE of the dispatch writes them -- the host has them tens of microseconds after
    // workgroup 0 has handed zeta back, so it does not wait, and its read over PCIe is not the kernel's tail (the last workgroup doing it was
    // measured: + 4 us on the kernel)
    if (ka.hosthead && ka.head_out != nullptr && wg == ((ka.nwg + 7) / 8) / 2 && wave < 2) {
        wait_tables(ka.hflag + 3, ka.seq, &sPoison);
        double* dst = wave == 0 ? ka.mean : ka.var;
        const double* src = ka.head_out + (wave == 0 ? 0 : ka.nhs);
        for (int t = lane; t < ka.nhs; t += 64) dst[t] = src[t];
    }
    acc = wave_sum_to_lane63(acc);
    if (lane == 63) sAcc[wave] = acc;
    TGP_STAMP(12);
    __syncthreads();
    TGP_STAMP(13);
    if (threadIdx.x == 0) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += sAcc[w];
        ka.part[wg] = t + sPoison;
        if (first) ka.part[ka.nwg] = head_quad;
        if (wg == ka.nwg - 1) ka.part[ka.nwg + 6] = (double)wall_clock64();
        if (probe) {
            ka.part[ka.nwg + 10] = (double)clock64();
            ka.part[ka.nwg + 11] = (double)wall_clock64();
        }
    }
}

// block-form helpers of the host side (the sign convention of the imaginary parts is preserved by squaring: re^2 - im^2, 2 re im)
static void bsquare(int d, const double* ar, const double* ai, double* outr, double* outi) {
    for (int i = 0; i < d; ++i) {
        const double r = ar[i] * ar[i] - ai[i] * ai[i], im = 2.0 * ar[i] * ai[i];
        outr[i] = r;
        outi[i] = im;
    }
}

template <int D>
void fill_args(KArgs<D>& ka, const Modal& md, int sub) {
    for (int i = 0; i < D; ++i) {
        ka.fd[i] = md.fd[i]; ka.fo[i] = md.fo[i]; ka.fb[i] = md.fb[i]; ka.fa[i] = md.fa[i]; ka.fw[i] = md.fw[i];
        ka.gd[i] = md.gd[i]; ka.go[i] = md.go[i]; ka.gc[i] = md.gc[i]; ka.gw[i] = md.gw[i];
        for (int j = 0; j < kWJ; ++j) {
            ka.WJ[j][i] = md.WJ[j][i];
            ka.WG[j][i] = md.WG[j][i];
        }
    }
    // in-tile scan levels M^(sub 2^k)
    if (sub == 8) {
        std::memcpy(ka.fpr[0], md.fp8r, sizeof(double) * D); std::memcpy(ka.fpi[0], md.fp8i, sizeof(double) * D);
        std::memcpy(ka.gpr[0], md.gp8r, sizeof(double) * D); std::memcpy(ka.gpi[0], md.gp8i, sizeof(double) * D);
    } else {
        bsquare(D, md.fp8r, md.fp8i, ka.fpr[0], ka.fpi[0]);
        bsquare(D, md.gp8r, md.gp8i, ka.gpr[0], ka.gpi[0]);
    }
    for (int k = 1; k < 6; ++k) {
        bsquare(D, ka.fpr[k - 1], ka.fpi[k - 1], ka.fpr[k], ka.fpi[k]);
        bsquare(D, ka.gpr[k - 1], ka.gpi[k - 1], ka.gpr[k], ka.gpi[k]);
    }
    // tile powers M^TILE, M^(2 TILE)
    if (sub == 8) {
        std::memcpy(ka.ftr[0], md.fp512r, sizeof(double) * D); std::memcpy(ka.fti[0], md.fp512i, sizeof(double) * D);
        std::memcpy(ka.gtr[0], md.gp512r, sizeof(double) * D); std::memcpy(ka.gti[0], md.gp512i, sizeof(double) * D);
    } else {
        bsquare(D, md.fp512r, md.fp512i, ka.ftr[0], ka.fti[0]);
        bsquare(D, md.gp512r, md.gp512i, ka.gtr[0], ka.gti[0]);
    }
    bsquare(D, ka.ftr[0], ka.fti[0], ka.ftr[1], ka.fti[1]);
    bsquare(D, ka.gtr[0], ka.gti[0], ka.gtr[1], ka.gti[1]);
    ka.hh = md.hh; ka.rS = md.rS; ka.vb = md.vb;
    ka.n0 = md.n0; ka.nhs = md.nhs; ka.halo = md.halo;
}

}  // namespace

struct Engine {
    HeadTables* tab = nullptr;      // host scratch of the plan
    double* hflat = nullptr;        // pinned host memory: the packed tables of the call (TabOff) + the flag word behind them
    double* dflat = nullptr;        // device memory: where workgroup 0 puts them
    size_t flat_cap = 0;            // doubles
    TabOff to{};
    size_t flat_used = 0;
    bool post = true;               // the launched call wants the posterior marginals (complete(): which stages of the tables)
    double* part = nullptr;         // pinned host memory
    size_t part_cap = 0;
    Modal md{};
    tgp_plan::Info info{};
    long long nwg = 0, seq = 0;      // workgroups of the whole series
    long long nwg_local = 0, wg0 = 0;      // ... of the last launch (a time segment runs a slice of them)
    bool owns_head = true;
    int nw = 8, sub = 8;
    bool began = false, deferred = false;
    // the head on the host (hosthead): pinned [0, 2 kHeadMax) head inputs y | Rnew, [2, 4 kHeadMax) head outputs mean | var, then z0 [8], zeta [8],
    // four flag words; hr: the head's innovations (host scratch)
    double* hhead = nullptr;
    double hr[tgp_plan::kHeadMax];
    bool hosthead = false, hh_pending = false;
    int rnew_per_step = 0;
    hipStream_t stream = nullptr;      // of the last launch (the host's waits watch it)
    double host_quad = 0.0;
    tgp_plan::ModelHost mh{};
    long long hh_T = 0;
    // the streaming logpdf kernel (tgp_lml.hip): a logpdf-only call over the whole series
    bool lml = false;
    tgp_lml::Geometry lg{};
    double lWt[tgp_plan::kMaxD * tgp_plan::kMaxD];
    void* lpart_raw = nullptr;         // (the block lpart lies in, as allocated)
    double* lpart = nullptr;           // pinned, on a 64-byte boundary, this kernel's alone: the workgroups' records as LINES (tgp_lml_record.hpp) and the TGP_LML_DBG stamps
    bool lml_records = false;          // the host may take the launched kernel's end from its records in pinned memory (tgp_lml.hpp records_there)
    // the streaming posterior kernel (tgp_post.hip): the last launch was k_post_stream (its sums are (value, check) records in `part`); the host
    // may take that launch's end from the records (every output byte written through and acknowledged in front of them: tgp_post.hpp records_end)
    bool post_stream = false, post_records = false;
    void* pxch = nullptr;              // device memory: the exchange records of the streaming posterior kernel's runs (tgp_post.hpp)
    long long stream_min_T = -1;       // TGP_OPT_STREAM_MIN_T
    // TGP_STEADY_DEBUG, a streaming call: the host's clock (steady_clock, ns) when it first saw a head observation, a record, the last record (0: never)
    long long dbg_ns[3] = {0, 0, 0};
    // the core of the last plan, kept while the model and the length stand (the reference's own sequence -- logpdf(model, y), then posterior(model, y) --
    // plans the same model twice): key = the model's blocks as handed over
    std::vector<double> memo_key;
    long long memo_T = -1;
    bool memo_ok = false;
    unsigned long long memo_stamp = 0; // of the thread's plan workspace when the core was built (another engine's plan on this thread, another thread: no hit)
    Modal memo_md{};
    // the input-normalised form of md the two streaming kernels run on (tgp_stream_form.hpp); !sf.ok: it declined, k_steady_one serves the call.  Built with
    // the plan's core and kept with it
    tgp_stream_form::Form sf{}, memo_sf{};
    tgp_plan::Info memo_info{};
    long long memo_Wt_n = -1;          // lWt holds quad_table(md, memo_Wt_n)
};
namespace {
constexpr size_t kHH = tgp_plan::kHeadMax;
inline double* hh_in(Engine* e) { return e->hhead; }
inline double* hh_out(Engine* e) { return e->hhead + 2 * kHH; }
inline double* hh_z0(Engine* e) { return e->hhead + 4 * kHH; }
inline double* hh_zeta(Engine* e) { return e->hhead + 4 * kHH + 8; }
inline long long* hh_flag(Engine* e) { return reinterpret_cast<long long*>(e->hhead + 4 * kHH + 16); }
// ... and behind the flags the same two states in the streaming kernels' coordinates: what k_post_stream reads and writes (k_steady_one: the plan's, above)
inline double* hh_kz0(Engine* e) { return e->hhead + 4 * kHH + 20; }
inline double* hh_kzeta(Engine* e) { return e->hhead + 4 * kHH + 28; }
constexpr size_t kHHDoubles = 4 * kHH + 36;

// ---- TGP_STEADY_DEBUG (read once): where a streaming call's time goes between the launch and the last record, on the host's clock.  In front of the
// launch head_in[0] is set to a word no series holds; the kernel's head wave replaces it first thing, so the first look that finds another word there
// has seen the kernel running.  await_done stamps the first and the last record.  (profiles/lml_call_tail_time.txt)
// Development only: both streaming kernels' head waves store head_in[0 .. nhs) in every launch, whatever the series' length, so the word is replaced before
// the head's forward recursion reads it; a launch that fails leaves it there, and the head then computed from it is discarded with the call's error.
inline bool steady_debug() {
    static const bool on = std::getenv("TGP_STEADY_DEBUG") != nullptr;
    return on;
}
inline long long host_ns() { return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
constexpr long long kDbgUnseen = 0x7FF8C0DEC0DEC0DEll;      // (a NaN with a payload of its own)
inline void dbg_arm(Engine* e) {
    e->dbg_ns[0] = e->dbg_ns[1] = e->dbg_ns[2] = 0;
    __atomic_store_n(reinterpret_cast<long long*>(hh_in(e)), kDbgUnseen, __ATOMIC_RELEASE);
}
inline void dbg_await_head(Engine* e) {      // (bounded by the stream, as await_host_flag is)
    const long long* p = reinterpret_cast<const long long*>(hh_in(e));
    for (unsigned spin = 1; __atomic_load_n(p, __ATOMIC_ACQUIRE) == kDbgUnseen; ++spin) {
        if ((spin & 4095u) == 0) {
            const hipError_t q = hipStreamQuery(e->stream);
            (void)hipGetLastError();
            if (q != hipErrorNotReady) return;
        }
        __builtin_ia32_pause();
    }
    e->dbg_ns[0] = host_ns();
}
}  // namespace
void debug_stamps(const Engine* e, long long ns[3]) {
    for (int k = 0; k < 3; ++k) ns[k] = e->dbg_ns[k];
}

Engine* create() { return new Engine(); }
void set_stream_min_T(Engine* e, long long v) {
    if (e) e->stream_min_T = v;
}
namespace {
// The streaming kernels' crossovers against k_steady_one (scripts/r06_kernel_T.py, d = 3: fixed 18 / 24 us + 0.7 / 2.9 us per 1e6 steps against
// 12 / 22 us + 1.9 / 3.8): below them the short-lived workgroups of k_steady_one finish first
constexpr long long kLmlMinT = 5000000, kPostMinT = 3000000;
inline bool stream_serves(const Engine* e, long long T, long long crossover) { return T >= (e->stream_min_T < 0 ? crossover : e->stream_min_T); }
}  // namespace
void destroy(Engine* e) {
    if (!e) return;
    delete e->tab;
    if (e->hflat) (void)tgp_alloc::host_free(e->hflat);
    if (e->hhead) (void)tgp_alloc::host_free(e->hhead);
    if (e->dflat) (void)tgp_alloc::dev_free(e->dflat);
    if (e->part) (void)tgp_alloc::host_free(e->part);
    if (e->lpart_raw) (void)tgp_alloc::host_free(e->lpart_raw);
    if (e->pxch) (void)tgp_alloc::dev_free(e->pxch);
    delete e;
}

const tgp_plan::Info& last_plan(const Engine* e) { return e->info; }
const char* kernel_name(const Engine* e, bool post) {
    if (e->lml && !post) return e->lg.n == 32 ? "k_lml_stream<32>" : "k_lml_stream<16>";
    return e->nw == 8 ? (post ? "k_steady_one<8x8,posterior>" : "k_steady_one<8x8,logpdf>") : (post ? "k_steady_one<16x8,posterior>" : "k_steady_one<16x8,logpdf>");
}
const tgp_plan::Modal& last_modal(const Engine* e) { return e->md; }

namespace {
static bool head_scans_enabled() {      // TGP_MODAL_HEAD_SCANS=0: the sequential head everywhere (A/B runs)
    static const bool on = [] {
        const char* v = std::getenv("TGP_MODAL_HEAD_SCANS");
        return !(v && v[0] == '0');
    }();
    return on;
}

// The streaming posterior kernel (tgp_post.hip) serves a call over the WHOLE series with the head on the host and every series-sized
// buffer on a 16-byte boundary; segments, in-kernel heads and odd pointers stay on k_steady_one.
static bool use_post_stream(const Engine* e, const Call& c) {
    if (c.mean == nullptr || !e->hosthead || c.seg_lo != 0 || (c.seg_hi >= 0 && c.seg_hi < c.T)) return false;
    if (!e->sf.ok || !tgp_post::applies(e->md, c.T) || !stream_serves(e, c.T, kPostMinT)) return false;
    auto al = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
    return al(c.y) && al(c.mean) && al(c.var) && (!c.rnew_per_step || al(c.Rnew));
}

// TGP_POST_RECORDS=0: the end of a k_post_stream launch by hipStreamSynchronize as before (A/B runs; the twin of TGP_LML_RECORDS).  The development
// stamps of TGP_POST_DBG are plain stores nobody waits for: they keep the synchronising end as well.
static bool post_records_enabled() {
    static const bool on = [] {
        const char* s = std::getenv("TGP_POST_RECORDS");
        return !(s && s[0] == '0') && std::getenv("TGP_POST_DBG") == nullptr;
    }();
    return on;
}

template <int D>
int launch(Engine* e, hipStream_t st, const Call& c, const char** kname) {
    if (use_post_stream(e, c)) {
        if (!e->pxch) {
            if (tgp_alloc::dev_malloc(&e->pxch, tgp_post::xch_bytes()) != hipSuccess) return (int)hipErrorOutOfMemory;
            if (hipMemsetAsync(e->pxch, 0, tgp_post::xch_bytes(), st) != hipSuccess) return (int)hipGetLastError();
        }
        const tgp_post::Geometry g = tgp_post::choose_geometry(e->sf.md, c.T);
        tgp_post::Call pc;
        pc.T = c.T;
        pc.y = c.y;
        pc.Rnew = c.Rnew;
        pc.rnew_per_step = c.rnew_per_step;
        pc.mean = c.mean;
        pc.var = c.var;
        pc.htab = e->hflat;
        pc.tvb_off = e->to.tvb;
        pc.flag = reinterpret_cast<const long long*>(e->hflat + e->flat_cap);
        pc.part = e->part;
        pc.head_in = hh_in(e);
        pc.z0p = hh_kz0(e);            // (the kernel's coordinates: `complete` maps the head's states on their way in and out)
        pc.zeta_out = hh_kzeta(e);
        pc.head_out = hh_out(e);
        pc.hflag = hh_flag(e);
        pc.seq = e->seq;
        pc.xch = e->pxch;
        e->post = true;
        e->rnew_per_step = c.rnew_per_step;
        e->stream = st;
        e->wg0 = 0;
        e->nwg_local = g.nwg;
        e->owns_head = true;
        e->hh_pending = true;
        e->post_stream = true;
        e->post_records = post_records_enabled() && tgp_post::records_end(pc);
        if (steady_debug()) dbg_arm(e);
        return tgp_post::enqueue(st, e->sf.md, g, pc, kname);
    }
    e->post_stream = false;
    KArgs<D> ka;
    static_assert(sizeof(KArgs<D>) <= 4096, "the kernel-argument segment");
    std::memset(&ka, 0, sizeof ka);
    fill_args<D>(ka, e->md, e->sub);
    ka.post = c.mean != nullptr ? 1 : 0;
    e->post = ka.post != 0;
    ka.rnew_per_step = c.rnew_per_step;
    ka.T = c.T;
    const int nw = e->nw, tile = 64 * e->sub;
    ka.C = (long long)nw * tile - 2LL * e->md.halo;
    // the launch's slice of the series' workgroups: all of them, or those that own outputs of the segment [seg_lo, seg_hi)
    const long long seg_lo = c.seg_lo, seg_hi = (c.seg_hi < 0 || c.seg_hi > c.T) ? c.T : c.seg_hi;
    const long long nhs = e->md.nhs;
    const long long g0 = seg_lo <= nhs ? 0 : (seg_lo - nhs) / ka.C, g1 = (seg_hi - nhs + ka.C - 1) / ka.C;
    e->wg0 = g0;
    e->nwg_local = g1 - g0;
    e->owns_head = seg_lo == 0;
    ka.nwg = e->nwg_local;
    ka.wg0 = g0;
    ka.seg_lo = seg_lo;
    ka.seg_hi = seg_hi;
    ka.T_eff = (seg_hi + e->md.halo < c.T) ? seg_hi + e->md.halo : c.T;
    ka.yl = c.yl;
    ka.yr = c.yr;
    ka.seq = e->seq;
    ka.y = c.y - seg_lo;
    ka.Rnew = c.Rnew;
    ka.RnewT = (c.Rnew && c.rnew_per_step) ? c.Rnew - seg_lo : c.Rnew;
    ka.mean = c.mean ? c.mean - seg_lo : nullptr;
    ka.var = c.var ? c.var - seg_lo : nullptr;
    ka.htab = e->hflat;
    ka.tab = e->dflat;
    ka.flag = reinterpret_cast<const long long*>(e->hflat + e->flat_cap);
    ka.to = e->to;
    ka.part = e->part;
    e->hh_pending = false;
    e->rnew_per_step = c.rnew_per_step;
    e->stream = st;
    if (e->hosthead && e->owns_head) {
        ka.hosthead = 1;
        ka.head_in = hh_in(e);
        ka.z0p = hh_z0(e);
        ka.zeta_out = hh_zeta(e);
        ka.head_out = ka.post ? hh_out(e) : nullptr;
        ka.hflag = hh_flag(e);
        e->hh_pending = true;
    }
    const long long per = (e->nwg_local + 7) / 8;
    const unsigned grid = (unsigned)(per * 8);
    *kname = kernel_name(e, ka.post != 0);
    // the head as scans (d <= 4) needs ~30 more registers per lane than the tiles' code: taken where the launch leaves the CUs room anyway
    // (at most two workgroups per CU: every series up to ~2e6 steps -- there the head IS the call), not where occupancy is the kernel's time
    const bool head_scans = D <= 4 && e->owns_head && e->nwg_local <= 512 && head_scans_enabled() && !ka.hosthead;
    if (nw == 8) {
        if (head_scans) hipLaunchKernelGGL((k_steady_one<D, 8, 8, (D <= 4)>), dim3(grid), dim3(8 * 64), 0, st, ka);
        else hipLaunchKernelGGL((k_steady_one<D, 8, 8, false>), dim3(grid), dim3(8 * 64), 0, st, ka);
    } else {
        hipLaunchKernelGGL((k_steady_one<D, 16, 8, false>), dim3(grid), dim3(16 * 64), 0, st, ka);
    }
    return (int)hipGetLastError();
}
}  // namespace

const char* kernel_name(const Engine* e, const Call& c) {
    if (use_post_stream(e, c)) return "k_post_stream";
    return kernel_name(e, c.mean != nullptr);
}

// TGP_MODAL_GEOMETRY=<waves>x<steps per lane> (8x8, 16x8) overrides the choice (A/B runs)
void choose_geometry(int d, int halo, int* nw, int* sub) {
    static const int forced = [] {
        const char* v = std::getenv("TGP_MODAL_GEOMETRY");
        int a = 0, b = 0;
        if (v && std::sscanf(v, "%dx%d", &a, &b) == 2 && b == 8 && (a == 8 || a == 16)) return a * 100 + b;
        return 0;
    }();
    const bool wide = 2 * halo * 10 > 3 * 4096;      // halos beyond ~30 % of a 4096-step span: spans of 8192 steps
    *sub = 8;
    *nw = wide ? 16 : 8;
    (void)d;
    if (forced) {
        *nw = forced / 100;
        *sub = forced % 100;
        if (halo * 2 >= *nw * 64 * *sub) {      // (a forced geometry too small for the halo: the wide default)
            *sub = 8;
            *nw = 16;
        }
    }
}

// This translation unit's host code is compiled for AVX2 + FMA (Makefile: the plan's small matrix products vectorise 4-wide -- an 8 x 8
// product 36 ns instead of 150); a host without them gets the five-launch engine.  (tgp_powers.hip, built with the same flags, asks here too.)
bool host_cpu_ok() {
    static const bool ok = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    return ok;
}

tgp_plan::Info plan_only(const tgp_plan::ModelHost& m, long long T, tgp_plan::Modal& md, tgp_plan::HeadTables& tab) {
    if (!host_cpu_ok()) {
        tgp_plan::Info in;
        in.why = tgp_plan::kEigFail;
        return in;
    }
    return tgp_plan::build_any(m, T, md, tab);
}

// TGP_MODAL_OVERLAP=0: the whole plan before the launch (A/B runs).  Also when the process runs with synchronous launches (the usual ROCm /
// PyTorch debugging switches): the kernel waits for flags the host raises AFTER hipLaunchKernelGGL returns -- a launch that does not return
// until the kernel has finished would wait for itself (round-4 advice; the wait is bounded as well, see wait_tables).
static bool hosthead_enabled() {      // TGP_MODAL_HOSTHEAD=0: the head inside the kernel as in round 4 (A/B runs)
    static const bool on = [] {
        const char* v = std::getenv("TGP_MODAL_HOSTHEAD");
        return !(v && v[0] == '0');
    }();
    return on;
}
static bool overlap_tables() {
    static const bool on = [] {
        const char* v = std::getenv("TGP_MODAL_OVERLAP");
        if (v && v[0] == '0') return false;
        for (const char* name : {"HIP_LAUNCH_BLOCKING", "CUDA_LAUNCH_BLOCKING", "AMD_SERIALIZE_KERNEL", "AMD_SERIALIZE_COPY"}) {
            const char* b = std::getenv(name);
            if (b && b[0] != '\0' && !(b[0] == '0' && b[1] == '\0')) return false;
        }
        return true;
    }();
    return on;
}

// the layout of the packed tables (fixed by d and n0: known when the kernel is launched, before the tables themselves)
static void layout_tables(Engine* e) {
    const int d = e->md.d, dd = d * d, n = e->md.n0 + 1;
    TabOff& to = e->to;
    int off = 1;
    auto take = [&](int cnt) {
        const int o = off;
        off += cnt;
        return o;
    };
    to.h = take(d);
    to.mu0 = take(d);
    to.Wm = take(dd);
    to.db = take(n * d);
    to.iS = take(n);
    to.rS = take(n);
    off += off & 1;                                   // (16-byte pieces)
    to.G = take(e->md.nhs * (dd + d));                // rows [G_t | c_t], one per head step t < nhs (steps behind n0: the stationary row)
    to.c = to.G;
    to.vb = take(n);
    to.tvb = take(0);
}

// packs one stage of the plan's tables for the device (pinned memory) and raises the stage's flag: 0 what the head's forward recursion
// reads, 1 the rows [G_t | c_t] of its backward recursion, 2 the smoothed variances of the head and of the last n1 steps.  A stage that
// declined (why != kOk) raises its flag and the later ones with the failure bit: the kernel never waits for a stage that will not come
static void ship_stage(Engine* e, int stage, int why) {
    const Modal& md = e->md;
    const HeadTables& tb = *e->tab;
    const int d = md.d, dd = d * d, n = md.n0 + 1;
    const TabOff& to = e->to;
    double* q = e->hflat;
    long long* hflag = reinterpret_cast<long long*>(e->hflat + e->flat_cap);
    if (why != tgp_plan::kOk) {
        for (int s2 = stage; s2 < 3; ++s2) __atomic_store_n(hflag + s2, 2 * e->seq + 1, __ATOMIC_RELEASE);
        return;
    }
    if (stage == 0) {
        std::memcpy(q + to.h, tb.h, sizeof(double) * d);
        std::memcpy(q + to.mu0, tb.mu0, sizeof(double) * d);
        std::memcpy(q + to.Wm, tb.Wm, sizeof(double) * dd);
        std::memcpy(q + to.db, tb.kA, sizeof(double) * n * d);
        std::memcpy(q + to.iS, tb.iS, sizeof(double) * n);
        std::memcpy(q + to.rS, tb.rS, sizeof(double) * n);
    } else if (stage == 1) {
        for (int t = 0; t < md.nhs; ++t) {
            const int tt = t < md.n0 ? t : md.n0;
            std::memcpy(q + to.G + (size_t)t * (dd + d), tb.G + (size_t)tt * dd, sizeof(double) * dd);
            std::memcpy(q + to.G + (size_t)t * (dd + d) + dd, tb.c + (size_t)tt * d, sizeof(double) * d);
        }
    } else {
        std::memcpy(q + to.vb, tb.vb, sizeof(double) * n);
        const int n1 = md.n1 > 0 ? md.n1 : 0;
        std::memcpy(q + to.tvb, tb.tvb, sizeof(double) * n1);
        q[0] = (double)n1;
        e->flat_used = (size_t)to.tvb + n1;
    }
    __atomic_store_n(hflag + stage, 2 * e->seq, __ATOMIC_RELEASE);
}

// the tables half of the plan, stage by stage, each shipped as soon as it exists.  Returns the Why of the first stage that declined
static int build_and_ship_tables(Engine* e, long long T, int nstages = 3) {
    e->memo_ok = false;      // (stage 0 rewrites the head's gains in place, in modal coordinates: the core in `tab` is no longer what build_core left)
    for (int stage = 0; stage < nstages; ++stage) {
        const int why = tgp_plan::build_tables_stage_any(e->md.d, stage, T, e->md, *e->tab, e->info);
        ship_stage(e, stage, why);
        if (why != tgp_plan::kOk) return why;
    }
    return tgp_plan::kOk;
}

static bool lml_stream_enabled() {      // TGP_LML_STREAM=0: logpdf on k_steady_one as in round 5 (A/B runs)
    static const bool on = [] {
        const char* v = std::getenv("TGP_LML_STREAM");
        return !(v && v[0] == '0');
    }();
    return on;
}

static bool lml_records_enabled() {      // TGP_LML_RECORDS=0: the end of a logpdf-only launch by hipStreamSynchronize as before (A/B runs)
    static const bool on = [] {
        const char* s = std::getenv("TGP_LML_RECORDS");
        return !(s && s[0] == '0');
    }();
    return on;
}
namespace {
bool plan_memo_enabled() {      // TGP_PLAN_MEMO=0: every call plans from scratch (A/B runs)
    static const bool on = [] {
        const char* s = std::getenv("TGP_PLAN_MEMO");
        return !(s && s[0] == '0');
    }();
    return on;
}
template <class F>
void model_words(const tgp_plan::ModelHost& m, F&& f) {
    const size_t d = (size_t)m.d;
    f(m.A, d * d); f(m.a, d); f(m.Q, d * d); f(m.H, d); f(m.hh, 1); f(m.R, 1); f(m.x0m, d); f(m.x0P, d * d);
}
bool memo_hit(const Engine* e, const tgp_plan::ModelHost& m, long long T) {
    if (!e->memo_ok || !plan_memo_enabled() || e->memo_T != T || e->memo_md.d != m.d) return false;
    if (tgp_plan::work_stamp_any(m.d) != e->memo_stamp) return false;      // (the stages behind the core read the thread's workspace: it must still be this plan's)
    const double* k = e->memo_key.data();
    bool same = true;
    model_words(m, [&](const double* p, size_t n) {
        same = same && std::memcmp(k, p, n * sizeof(double)) == 0;
        k += n;
    });
    return same;
}
void memo_store(Engine* e, const tgp_plan::ModelHost& m, long long T) {
    e->memo_key.clear();
    model_words(m, [&](const double* p, size_t n) { e->memo_key.insert(e->memo_key.end(), p, p + n); });
    e->memo_T = T;
    e->memo_md = e->md;
    e->memo_sf = e->sf;
    e->memo_info = e->info;
    e->memo_stamp = tgp_plan::work_stamp_any(m.d);
    e->memo_ok = true;
}
}  // namespace
bool plan(Engine* e, const tgp_plan::ModelHost& m, long long T, bool logpdf_only) {
    e->began = false;
    e->lml = false;
    e->post_stream = false;
    if (!host_cpu_ok()) {
        e->info = tgp_plan::Info{};
        e->info.why = tgp_plan::kEigFail;
        return false;
    }
    if (!e->tab) {
        e->tab = new HeadTables();
        // the layout of ship_tables at its largest: d = 8, n0 = kN0Max, n1 = kTailMax
        e->flat_cap = (size_t)tgp_plan::kHeadMax * (64 + 8) + (size_t)(tgp_plan::kN0Max + 1) * (8 + 3) + tgp_plan::kTailMax + 64 + 2 * 8 + 8;
        e->flat_cap = (e->flat_cap + 1) & ~(size_t)1;
        if (tgp_alloc::host_malloc(reinterpret_cast<void**>(&e->hflat), (e->flat_cap + 4) * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess ||
            tgp_alloc::dev_malloc(reinterpret_cast<void**>(&e->dflat), (e->flat_cap + 4) * sizeof(double)) != hipSuccess) {
            e->info = tgp_plan::Info{};
            e->info.why = tgp_plan::kEigFail;
            return false;
        }
        for (int s2 = 0; s2 < 3; ++s2) reinterpret_cast<long long*>(e->hflat + e->flat_cap)[s2] = 0;      // (the stages' flags)
    }
    if (!e->hhead) {
        const size_t n = kHHDoubles;
        if (tgp_alloc::host_malloc(reinterpret_cast<void**>(&e->hhead), n * sizeof(double), hipHostMallocCoherent | hipHostMallocMapped) != hipSuccess) {
            e->info = tgp_plan::Info{};
            e->info.why = tgp_plan::kEigFail;
            return false;
        }
        std::memset(e->hhead, 0, n * sizeof(double));
    }
    ++e->seq;
    if (memo_hit(e, m, T)) {
        e->md = e->memo_md;
        e->sf = e->memo_sf;
        e->info = e->memo_info;
    } else {
        e->memo_ok = false;
        e->memo_Wt_n = -1;
        e->info = tgp_plan::build_core_any(m, T, e->md, *e->tab);
        if (e->info.why != tgp_plan::kOk) return false;
        (void)tgp_stream_form::build(e->md, e->sf);
        memo_store(e, m, T);
    }
    layout_tables(e);
    e->mh = m;
    e->hh_T = T;
    if (logpdf_only && e->sf.ok && e->sf.amp <= tgp_stream_form::kClosureAmpMax && lml_stream_enabled() && stream_serves(e, T, kLmlMinT)) {
        // the streaming logpdf kernel: no tables (the head runs on the host from build_core's gains), no wait inside the kernel
        e->lg = tgp_lml::choose_geometry(e->sf.md, T);
        if (!e->lpart) {
            // the records' own area (its lines never mix with the pair records of k_post_stream in `part`), the largest table and the development stamps
            // of TGP_LML_DBG; cleared: the allocator hands out parked pinned blocks as they were left, and a zeroed line passes for no call's
            // (a line is ONE aligned 64-byte write: the area starts on the block's first 64-byte boundary, wherever the allocator's block starts)
            const size_t need = (tgp_lml::part_doubles(e->md.d) + 64) * sizeof(double);
            if (tgp_alloc::host_malloc(&e->lpart_raw, need + 64, hipHostMallocDefault) != hipSuccess) {
                e->lpart_raw = nullptr;
                e->info.why = tgp_plan::kEigFail;
                return false;
            }
            std::memset(e->lpart_raw, 0, need + 64);
            e->lpart = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(e->lpart_raw) + 63) & ~(uintptr_t)63);
        }
        if (e->memo_Wt_n != e->lg.first_tile) {
            tgp_lml::quad_table(e->sf.md, e->lg.first_tile, e->lWt);      // (in the kernel's coordinates, like its records)
            e->memo_Wt_n = e->memo_ok ? e->lg.first_tile : -1;
        }
        e->deferred = false;
        e->hosthead = false;
        e->lml = true;
        e->nwg = e->lg.nwg;
        e->began = true;
        return true;
    }
    // the tables half: behind the launch when the series is certainly longer than head + tail (the kernel's head wave and last tiles wait
    // for the flag), else right here
    // (measured again in round 5, d = 3: with the tables behind the launch a call takes 63.5 us against 68.7 with them in front of it, the
    //  kernel 47 us either way: scripts/call_overhead.py; TGP_MODAL_OVERLAP=0 is the switch)
    e->deferred = overlap_tables() && T >= (long long)e->md.nhs + tgp_plan::kTailMax + 1;
    // the head on the host wherever the tables may follow the launch: workgroup 0 waits for the head's end state, not for tables
    e->hosthead = e->deferred && hosthead_enabled();
    if (!e->deferred) {
        const int why = build_and_ship_tables(e, T);
        if (why != tgp_plan::kOk) {
            e->info.why = why;
            return false;
        }
    }
    // geometry: steps per lane (8 or 16) and tiles per workgroup; spans of 4096 steps unless the halos would eat more than ~30 % of them, then 8192
    const int halo = e->md.halo;
    choose_geometry(e->md.d, halo, &e->nw, &e->sub);
    const long long C = (long long)e->nw * 64 * e->sub - 2LL * halo;
    e->nwg = (T - e->md.nhs + C - 1) / C;
    // (k_steady_one: a sum per workgroup and its development stamps; k_post_stream: its record table and stamps)
    const size_t need = std::max<size_t>({(size_t)e->nwg + 64, tgp_post::part_doubles(), (size_t)8192});
    if (need > e->part_cap) {
        if (e->part) (void)tgp_alloc::host_free(e->part);
        e->part = nullptr;
        e->part_cap = 0;
        if (tgp_alloc::host_malloc(reinterpret_cast<void**>(&e->part), need * sizeof(double), hipHostMallocDefault) != hipSuccess) {
            e->info.why = tgp_plan::kEigFail;
            return false;
        }
        // (cleared as the logpdf path clears its own: the allocator hands out parked pinned blocks as they were left, and another engine's records
        //  -- its call numbers start at 1 as this one's do -- must not pass for this engine's in await_done)
        std::memset(e->part, 0, need * sizeof(double));
        e->part_cap = need;
    }
    e->began = true;
    return true;
}

// The host's side of a hand-over: spins on a flag in pinned memory the kernel raises.  Not bounded by the clock -- the kernel may not even
// have started (a stream with work of the caller's in front of it) -- but by the stream: once it has drained (hipStreamQuery, every few
// thousand spins) the kernel is through, and the flag is there or will never be (the kernel's own waits give up after two seconds and
// poison its result).  false: the stream is done, or in error, and the flag never came.
bool await_host_flag(const long long* f, long long v, hipStream_t stream) {
    for (unsigned spin = 1;; ++spin) {
        if (__atomic_load_n(f, __ATOMIC_ACQUIRE) >= v) return true;
        if ((spin & 4095u) == 0) {
            const hipError_t q = hipStreamQuery(stream);
            (void)hipGetLastError();      // (hipErrorNotReady is not an error of ours: it must not surface in the next launch's check)
            if (q != hipErrorNotReady) return __atomic_load_n(f, __ATOMIC_ACQUIRE) >= v;
        }
        __builtin_ia32_pause();
    }
}
namespace {
void raise_flag(long long* f, long long v) {
    if (__atomic_load_n(f, __ATOMIC_RELAXED) < v) __atomic_store_n(f, v, __ATOMIC_RELEASE);
}
}  // namespace

// Behind the launch: the tables half of the plan, if it was deferred.  false: it declined (the kernel has been released all the same -- whatever
// it writes is to be discarded, the caller re-runs the call elsewhere after synchronising).
bool complete(Engine* e, long long T) {
    if (e->began && e->lml) {
        // the head's forward recursion, as soon as the kernel has handed its observations over (or the stream has drained)
        // (false: the stream has drained without the flag -- a short series, whose head wave raises none: the kernel's end has delivered the data.
        //  A launch that failed is the caller's stream synchronisation's to report; the head of garbage is then discarded with the rest)
        if (steady_debug()) dbg_await_head(e);
        (void)await_host_flag(hh_flag(e), 2 * e->seq, e->stream);
        tgp_plan::modal_head_forward_any(e->mh, e->md, *e->tab, hh_in(e), e->hr, hh_z0(e), &e->host_quad);
        return true;
    }
    if (!e->began || !e->deferred) return true;
    e->deferred = false;
    if (!e->hosthead) {
        const int why = build_and_ship_tables(e, T, e->post ? 3 : 1);      // (a logpdf-only launch reads the forward stage alone)
        if (why != tgp_plan::kOk) {
            e->info.why = why;
            return false;
        }
        return true;
    }
    // ---- the head on the host: its forward recursion as soon as workgroup 0 has handed the observations over, the tables of stages 1 and 2
    // beside the kernel (stage 2 is shipped: the last tiles read the tail variances), the backward recursion once the kernel has handed zeta back
    long long* f = hh_flag(e);
    const long long v = 2 * e->seq;
    const bool head = e->hh_pending;
    e->hh_pending = false;
    bool ok = true;
    int why = tgp_plan::kOk;
    // the tail variances FIRST (round 6): the runs / workgroups at the series' end wait for them from the moment they start, and they need nothing of
    // the head (measured on k_post_stream: shipped behind the head's tables they left the series' last run waiting until 50 us into a 35 us kernel)
    if (e->post) {
        why = tgp_plan::build_tables_tail_any(e->md.d, T, e->md, *e->tab, e->info);
        ship_stage(e, 2, why);      // (the head's variances in that stage are not there yet: with the head on the host nobody on the device reads them)
    }
    if (head) {
        if (steady_debug() && e->post_stream) dbg_await_head(e);      // (behind the tail's tables: seen no later than this)
        ok = await_host_flag(f, v, e->stream);
        if (ok) tgp_plan::modal_head_forward_any(e->mh, e->md, *e->tab, hh_in(e), e->hr, hh_z0(e), &e->host_quad);
        if (ok && e->post_stream) tgp_stream_form::state_in(e->sf, hh_z0(e), hh_kz0(e));
        raise_flag(f + 1, v);
    }
    if (e->post && why == tgp_plan::kOk) {
        why = tgp_plan::build_tables_stage_any(e->md.d, 1, T, e->md, *e->tab, e->info);
        if (why == tgp_plan::kOk) why = tgp_plan::build_tables_headvar_any(e->md.d, e->md, *e->tab);
    }
    if (head && e->post) {
        if (ok && why == tgp_plan::kOk) ok = await_host_flag(f + 2, v, e->stream);
        if (ok && why == tgp_plan::kOk) {
            const int nhs = e->md.nhs;
            double *om = hh_out(e), *ov = om + nhs;
            const double* in = hh_in(e);
            if (e->post_stream) tgp_stream_form::zeta_out(e->sf, hh_kzeta(e), hh_zeta(e));
            tgp_plan::modal_head_backward_any(e->md, *e->tab, in, e->hr, hh_zeta(e), om, ov);
            for (int t = 0; t < nhs; ++t) ov[t] += in[nhs + (e->rnew_per_step ? t : 0)];
        }
        raise_flag(f + 3, v);      // (also when something declined: the last workgroup never waits for what will not come; the outputs are discarded)
    }
    if (why != tgp_plan::kOk) {
        e->info.why = why;
        return false;
    }
    if (!ok) {
        e->info.why = tgp_plan::kEigFail;      // (the host / device hand-over timed out)
        return false;
    }
    return true;
}

// The kernel of a logpdf-only call produces nothing but the workgroups' records in pinned memory, each 64-byte line of them marked with the call's key: once
// every record is there the kernel has read all of y and written all it writes, and the host goes on without hipStreamSynchronize (the kernel's own
// end -- the release at the end of the dispatch, the queue's barrier packet, the completion signal -- is ~4 us the caller need not wait for; the
// stream stays ordered: whatever is enqueued next runs behind the kernel).  false: the stream drained or failed without them -- synchronise.
// k_post_stream takes the same end: its workgroups store mean and var write-through and issue their record -- one pair each -- behind the last
// acknowledged output store of their waves, so with every record there the outputs are in memory for any stream of the device.  Launches that keep
// plain stores -- a noise variance per step -- and every k_steady_one launch, segments included, synchronise as before.
bool await_done(Engine* e) {
    if (!e || !e->began) return false;
    if (e->lml ? !e->lml_records : !(e->post_stream && e->post_records)) return false;
    // (the logpdf kernel's records are lines in its own area, checked a line at a time; the posterior kernel's are pairs, one per workgroup)
    const size_t n = e->lml ? (size_t)e->lg.nwg * tgp_lml::record_lines(e->md.d) : (size_t)e->nwg_local;
    auto there = [&](size_t* next) { return e->lml ? tgp_lml::records_there(e->lg, e->md.d, e->lpart, e->seq, next) : tgp_lml::records_there(n, e->part, e->seq, next); };
    size_t next = 0;
    const bool dbg = steady_debug();
    for (unsigned spin = 1;; ++spin) {
        if (dbg && e->dbg_ns[1] == 0) {      // (any record of this call, whichever workgroup's)
            const unsigned long long key = tgp_lml::record_key(e->seq);
            const volatile unsigned long long* q = reinterpret_cast<const volatile unsigned long long*>(e->lml ? e->lpart : e->part);
            for (size_t k = 0; k < n && e->dbg_ns[1] == 0; ++k)
                if (e->lml ? tgp_lml::record_line_ok(q + k * tgp_lml::kLineWords, key) : (q[2 * k] ^ q[2 * k + 1]) == key) e->dbg_ns[1] = host_ns();
        }
        if (there(&next)) {
            if (dbg) e->dbg_ns[2] = host_ns();
            return true;
        }
        if ((spin & 4095u) == 0) {
            const hipError_t q = hipStreamQuery(e->stream);
            (void)hipGetLastError();
            if (q != hipErrorNotReady) return there(&next);
        }
        __builtin_ia32_pause();
    }
}

// A caller that leaves between enqueue() and complete() (an error return in between) must not leave the kernel waiting: raises the flags of
// a deferred plan with the failure bit (what the kernel writes is then discarded by whoever reads it).  Harmless otherwise.
void abandon(Engine* e) {
    if (!e || !e->began || !e->deferred || !e->hflat) return;
    e->deferred = false;
    long long* hflag = reinterpret_cast<long long*>(e->hflat + e->flat_cap);
    for (int s2 = 0; s2 < 3; ++s2) __atomic_store_n(hflag + s2, 2 * e->seq + 1, __ATOMIC_RELEASE);
    if (e->hhead) {
        raise_flag(hh_flag(e) + 1, 2 * e->seq);
        raise_flag(hh_flag(e) + 3, 2 * e->seq);
    }
    e->hh_pending = false;
}

int enqueue(Engine* e, hipStream_t stream, const Call& c, const char** kname, std::string* err) {
    if (!e || !e->began || !c.y || c.T <= 0 || (c.mean && (!c.var || !c.Rnew))) {
        if (err) *err = "tgp_modal::enqueue: bad argument / no plan";
        return (int)hipErrorInvalidValue;
    }
    int r = 0;
    if (e->lml) {
        if (c.mean != nullptr || c.seg_lo != 0 || (c.seg_hi >= 0 && c.seg_hi < c.T)) {
            if (err) *err = "tgp_modal::enqueue: the plan was made for a logpdf-only call over the whole series";
            return (int)hipErrorInvalidValue;
        }
        tgp_lml::Buffers b;
        b.part = e->lpart;
        b.head_in = hh_in(e);
        b.flags = hh_flag(e);
        e->lml_records = lml_records_enabled();
        e->post_stream = false;
        e->post = false;
        e->stream = stream;
        e->owns_head = true;
        e->nwg_local = e->lg.nwg;
        if (steady_debug()) dbg_arm(e);
        r = tgp_lml::enqueue(stream, e->sf.md, e->lg, c.T, c.y, b, e->seq, e->lWt, kname);
        if (r != 0 && err) *err = std::string("tgp_lml: launch: ") + hipGetErrorString((hipError_t)r);
        return r;
    }
    switch (e->md.d) {
        case 1: r = launch<1>(e, stream, c, kname); break;
        case 2: r = launch<2>(e, stream, c, kname); break;
        case 3: r = launch<3>(e, stream, c, kname); break;
        case 4: r = launch<4>(e, stream, c, kname); break;
        case 5: r = launch<5>(e, stream, c, kname); break;
        case 6: r = launch<6>(e, stream, c, kname); break;
        case 7: r = launch<7>(e, stream, c, kname); break;
        case 8: r = launch<8>(e, stream, c, kname); break;
        default: r = (int)hipErrorInvalidValue;
    }
    if (r != 0 && err) *err = std::string("tgp_modal: launch: ") + hipGetErrorString((hipError_t)r);
    return r;
}

// After the stream has passed the kernel: the launch's share of the quadratic form -- the sum of r^2 over the steps it owns behind the head
// and (the launch that holds the head) the head's sum of r^2 / S_t; fixed summation order.
void finish_parts(const Engine* e, double* ssq, double* head_quad) {
    if (e->lml) {
        double z0k[tgp_plan::kMaxD];      // the head's end state as the records see it
        tgp_stream_form::state_in(e->sf, e->hhead + 4 * kHH, z0k);
        *ssq = tgp_lml::finish(e->sf.md, e->lg, e->lpart, z0k, e->lWt);
        *head_quad = e->host_quad;
        return;
    }
    double s = 0.0;
    const int stride = e->post_stream ? 2 : 1;      // (k_post_stream: (value, check) pairs)
    for (long long g = 0; g < e->nwg_local; ++g) s += e->part[stride * g];
    *ssq = s;
    *head_quad = e->owns_head ? (e->hosthead ? e->host_quad : e->part[e->nwg_local]) : 0.0;
}

// ... and the log marginal likelihood of a call that ran the whole series.
double finish(const Engine* e, long long T) {
    const Modal& md = e->md;
    if (std::getenv("TGP_POST_DBG") != nullptr && (std::atoi(std::getenv("TGP_POST_DBG")) & 16) && e->post && e->nwg_local <= 256) {
        // development: the runs' start / end stamps of k_post_stream (100 MHz ticks)
        const double* q = e->part + tgp_post::kStampOff;
        const long long R = e->nwg_local * 8;
        double s0 = 1e300, s1 = -1e300, e0 = 1e300, e1 = -1e300, esum = 0.0;
        long long elast = -1, n = 0;
        for (long long r = 0; r < R; ++r) {
            if (q[2 * r] == 0.0) continue;
            ++n;
            s0 = std::min(s0, q[2 * r]); s1 = std::max(s1, q[2 * r]);
            e0 = std::min(e0, q[2 * r + 1]);
            esum += q[2 * r + 1];
            if (q[2 * r + 1] > e1) { e1 = q[2 * r + 1]; elast = r; }
        }
        {
            // histogram of the ends (2 us bins), mean end by XCD (workgroup number mod 8) and by wave slot
            int hist[64] = {0};
            double xs[8] = {0}, ws[8] = {0};
            int xn[8] = {0}, wn[8] = {0};
            for (long long r = 0; r < R; ++r) {
                if (q[2 * r] == 0.0) continue;
                const double en = (q[2 * r + 1] - s0) * 0.01;
                const int b = (int)(en / 2.0);
                ++hist[b < 63 ? b : 63];
                xs[(r / 8) % 8] += en; ++xn[(r / 8) % 8];
                ws[r % 8] += en; ++wn[r % 8];
            }
            fprintf(stderr, "[tgp post] ends by 2 us:");
            for (int b = 0; b < 40; ++b) if (hist[b]) fprintf(stderr, " %d:%d", 2 * b, hist[b]);
            fprintf(stderr, "\n[tgp post] mean end by XCD:");
            for (int x = 0; x < 8; ++x) fprintf(stderr, " %.1f", xs[x] / std::max(1, xn[x]));
            fprintf(stderr, "; by wave of the workgroup:");
            for (int x = 0; x < 8; ++x) fprintf(stderr, " %.1f", ws[x] / std::max(1, wn[x]));
            fprintf(stderr, "\n");
        }
        fprintf(stderr, "[tgp post] %lld runs: starts within %.2f us; ends: first %.2f, mean %.2f, last %.2f us after the first start (run %lld); run 0 ends %.2f, run R/2 ends %.2f\n", n,
                (s1 - s0) * 0.01, (e0 - s0) * 0.01, (esum / n - s0) * 0.01, (e1 - s0) * 0.01, elast, (q[1] - s0) * 0.01, (q[2 * (R / 2) + 1] - s0) * 0.01);
    }
    if (e->lml && std::getenv("TGP_LML_DBG") != nullptr) {
        const double* q = e->lpart + tgp_lml::kStampOff;
        double s0 = 1e300, s1 = 0, l1 = 0, c1 = 0, b1 = 0, e1 = 0;
        for (int g = 0; g < e->lg.nwg && g < 512; ++g) {
            s0 = std::min(s0, q[8 * g]);
            s1 = std::max(s1, q[8 * g]);
        }
        for (int g = 0; g < e->lg.nwg && g < 512; ++g) {
            l1 = std::max(l1, q[8 * g + 1] - s0); c1 = std::max(c1, q[8 * g + 2] - s0); b1 = std::max(b1, q[8 * g + 3] - s0); e1 = std::max(e1, q[8 * g + 4] - s0);
        }
        fprintf(stderr, "[tgp lml] %d workgroups; wave 0 of each, us after the first start: starts within %.2f; first tile landed by %.2f; runs done by %.2f; barrier passed by %.2f; triples written by %.2f\n",
                e->lg.nwg, (s1 - s0) * 0.01, l1 * 0.01, c1 * 0.01, b1 * 0.01, e1 * 0.01);
    }
    if (!e->lml && std::getenv("TGP_STEADY_DEBUG") != nullptr) {
        const double* q = e->part + e->nwg_local;
        fprintf(stderr, "[tgp modal] d %d n0 %d nhs %d n1 %d halo %d geometry %dx%d workgroups %lld | workgroup 0 (us from its start): tables ready %.1f, head forward done %.1f, head backward starts %.1f, done %.1f; last workgroup done %.1f\n",
                md.d, md.n0, md.nhs, md.n1, md.halo, e->nw, e->sub, e->nwg_local, (q[2] - q[1]) * 0.01, (q[3] - q[1]) * 0.01, (q[4] - q[1]) * 0.01, (q[5] - q[1]) * 0.01, (q[6] - q[1]) * 0.01);
        if (q[11] > q[9])
            fprintf(stderr, "[tgp modal] a mid-series workgroup lived %.2f us = %.0f shader cycles (%.0f MHz); it started %.1f us after workgroup 0\n", (q[11] - q[9]) * 0.01, q[10] - q[8],
                    (q[10] - q[8]) / ((q[11] - q[9]) * 0.01), (q[9] - q[1]) * 0.01);
#ifdef TGP_MODAL_PROBE
        {
            static const char* nm[14] = {"entry", "y loaded", "forward steps", "forward scan", "barrier 1", "corrections", "backward steps", "backward scan", "barrier 2", "mean rows in LDS",
                                         "mean stores issued", "variance stores issued", "wave sum", "barrier 3"};
            fprintf(stderr, "[tgp modal] phases of its wave 0 (shader cycles since entry):");
            for (int k = 1; k < 14; ++k) fprintf(stderr, " %s %.0f;", nm[k], q[12 + k] - q[12]);
            fprintf(stderr, "\n[tgp modal] its waves reached barrier 1 at");
            for (int w = 0; w < e->nw; ++w) fprintf(stderr, " %.0f", q[28 + w] - q[12]);
            fprintf(stderr, "; barrier 2 at");
            for (int w = 0; w < e->nw; ++w) fprintf(stderr, " %.0f", q[28 + e->nw + w] - q[12]);
            fprintf(stderr, "\n");
        }
#endif
    }
    double s = 0.0, hq = 0.0;
    finish_parts(e, &s, &hq);
    const double quad = hq + md.iS * s;
    const double logdet = md.LS + (double)(T - md.n0) * md.logS;
    return -0.5 * ((double)T * kLog2Pi + logdet + quad);
}

bool overlap_allowed() { return overlap_tables(); }

}  // namespace tgp_modal
