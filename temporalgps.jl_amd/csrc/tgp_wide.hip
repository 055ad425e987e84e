// Stationary-gain engine for wide states (8 < d <= 63) -- see tgp_wide.hpp.  gfx950 only (wave64).
#include "tgp_wide.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "tgp_alloc.hpp"
#include "tgp_lane.hpp"
#include "tgp_wide_adjoint_host.hpp"

namespace tgp_wide {

namespace {

struct ZArg {
    double z[64];      // the filtered mean behind the head, one component per lane (zero beyond d)
};

// the LDS kernels' inner product: a0 + (the lane's row phi) . (the state in the LDS line zb), on four accumulator chains
template <int DP>
__device__ __forceinline__ double lds_dot(const double (&phi)[DP], const double* zb, double a0) {
    double a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int j = 0; j < DP; j += 8) {
        const v2d q0 = *reinterpret_cast<const v2d*>(&zb[j]), q1 = *reinterpret_cast<const v2d*>(&zb[j + 2]);
        const v2d q2 = *reinterpret_cast<const v2d*>(&zb[j + 4]), q3 = *reinterpret_cast<const v2d*>(&zb[j + 6]);
        a0 = fma(phi[j], q0.x, a0);
        a1 = fma(phi[j + 1], q0.y, a1);
        a2 = fma(phi[j + 2], q1.x, a2);
        a3 = fma(phi[j + 3], q1.y, a3);
        a0 = fma(phi[j + 4], q2.x, a0);
        a1 = fma(phi[j + 5], q2.y, a1);
        a2 = fma(phi[j + 6], q3.x, a2);
        a3 = fma(phi[j + 7], q3.y, a3);
    }
    return (a0 + a1) + (a2 + a3);
}
// the smoothed emission variance of step t behind the head (see k_wide_bwd): a constant but for the last n1 steps, plus the replaced noise
__device__ __forceinline__ void store_var(double* __restrict__ var, long long t, long long T, const double* __restrict__ qtab, long long n1, double vbase, double qinf,
                                          const double* __restrict__ Rnew, int rnew_per_step) {
    const long long jt = T - 1 - t;
    const double q = jt < n1 ? qtab[jt] : qinf;
    var[t] = vbase - q + (rnew_per_step ? Rnew[t] : Rnew[0]);
}

// tab: [DP + 2][64] -- column j of the lanes' rows (lane i < d: row i of Phi; lane d: -g; zero beyond), then the lanes' input gains (K_i; 1 for the
// observer) and constants (c_i; -g0 for the observer).  One wave per chunk [s0, s1) of the steps behind the head; its warm-up starts `halo` steps
// early from zero, or at the head's end from the head's own end state where that is nearer.
template <int DP>
__global__ __launch_bounds__(64) void k_wide_lml(const double* __restrict__ tab, const double* __restrict__ y, double hh, long long T, long long t_head,
                                                  long long chunk_len, long long halo, int obs_lane, ZArg z0, double* __restrict__ part, double* __restrict__ rout,
                                                  const double* __restrict__ ht, double* __restrict__ mout, int d) {
    __shared__ __attribute__((aligned(16))) double zb[64];
    const int lane = threadIdx.x;
    const long long chunk = blockIdx.x;
    const long long s0 = t_head + chunk * chunk_len;
    long long s1 = s0 + chunk_len;
    if (s1 > T) s1 = T;
    // (ht: an emission offset PER STEP -- a mean function at the inputs -- instead of the shared hh: the gains do not see it)
    auto obs = [&](long long t) { return y[t] - (ht != nullptr ? ht[t] : 0.0); };
    const bool from_head = s0 - halo <= t_head;
    const long long w0 = from_head ? t_head : s0 - halo;
    double phi[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) phi[j] = tab[(size_t)j * 64 + lane];
    const double kin = tab[(size_t)DP * 64 + lane], cin = tab[(size_t)(DP + 1) * 64 + lane];
    zb[lane] = from_head ? z0.z[lane] : 0.0;
    lds_sync();
    double ssq = 0.0;
    double yn = (w0 + lane < s1) ? obs(w0 + lane) : 0.0;
    for (long long tb = w0; tb < s1; tb += 64) {
        const double yv = yn;
        yn = (tb + 64 + lane < s1) ? obs(tb + 64 + lane) : 0.0;      // (the next block's observations: on their way while this block runs)
        const int nb = (int)((s1 - tb < 64) ? (s1 - tb) : 64);
        const bool keep = rout != nullptr && tb + 64 > s0;          // (a posterior call: the innovations of the chunk's own steps go to memory)
        double outr = 0.0;
        for (int l = 0; l < nb; ++l) {
            const double u = readlane_d(yv, l) - hh;
            const double acc = lds_dot<DP>(phi, zb, fma(kin, u, cin));
            lds_sync();      // (every lane has read the old state)
            zb[lane] = acc;
            lds_sync();
            if (tb + l >= s0) ssq = fma(acc, acc, ssq);      // (the observer's acc is the step's innovation)
            if (mout != nullptr && tb + l >= s0 && lane < d) mout[(tb + l) * d + lane] = acc;      // (_filter: the filtered mean of the chunk's own steps)
            if (keep) {
                const double rr = readlane_d(acc, obs_lane);
                outr = lane == l ? rr : outr;
            }
        }
        if (keep && lane < nb && tb + lane >= s0) rout[tb + lane] = outr;
    }
    const double s = readlane_d(ssq, obs_lane);
    if (lane == 0) part[chunk] = s;
}

// The backward half (Bryson-Frazier in the predicted form): lam_t = h r_t / S + Psi lam_(t+1), Psi = (I - h K') A';
// mean_t = y_t - (R / S) r_t + gw . lam_(t+1), gw = R A K; var_t = (S - R) R / S - gw' Lam_(t+1) gw + Rnew_t, where the quadratic form is a constant
// behind the last n1 steps (qtab: its partial sums at the series' end).  tab: [DP + 1][64] -- column j of the lanes' rows (lane i < d: row i of Psi;
// lane d, the observer: gw), then the gains on r_t (h_i / S; observer: -R / S).  A chunk starts `halo` steps behind its end from lam = 0 (exact at T).
// ADJ (the adjoint pass of logpdf, tgp_wide::adjoint): lam_t of the chunk's own steps to lamT [T][d] instead of the means and variances -- lam_t is
// d logpdf / d mu_t, mu_t the predicted mean (the observer's row is not used).
template <int DP, bool ADJ = false>
__global__ __launch_bounds__(64) void k_wide_bwd(const double* __restrict__ tab, const double* __restrict__ y, const double* __restrict__ r,
                                                  const double* __restrict__ Rnew, int rnew_per_step, const double* __restrict__ qtab, long long n1, double vbase,
                                                  double qinf, long long T, long long t_head, long long chunk_len, long long halo, int obs_lane, int d,
                                                  double* __restrict__ mean, double* __restrict__ var, double* __restrict__ lam_out, double* __restrict__ lamT) {
    __shared__ __attribute__((aligned(16))) double zb[64];
    const int lane = threadIdx.x;
    const long long chunk = blockIdx.x;
    const long long s0 = t_head + chunk * chunk_len;
    long long s1 = s0 + chunk_len;
    if (s1 > T) s1 = T;
    long long w1 = s1 + halo;
    if (w1 > T) w1 = T;
    double phi[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) phi[j] = tab[(size_t)j * 64 + lane];
    const double kin = tab[(size_t)DP * 64 + lane];
    zb[lane] = 0.0;
    lds_sync();
    double rn = (w1 - 1 - lane >= s0) ? r[w1 - 1 - lane] : 0.0;
    for (long long tb = w1 - 1; tb >= s0; tb -= 64) {      // the block holds the steps tb, tb - 1, ..., one per lane
        const double rv = rn;
        rn = (tb - 64 - lane >= s0) ? r[tb - 64 - lane] : 0.0;
        const int nb = (int)((tb - s0 + 1 < 64) ? (tb - s0 + 1) : 64);
        const bool own = tb - 63 < s1;      // (some step of the block is the chunk's own)
        double outm = 0.0;
        for (int l = 0; l < nb; ++l) {
            const double acc = lds_dot<DP>(phi, zb, kin * readlane_d(rv, l));
            lds_sync();
            zb[lane] = acc;
            lds_sync();
            if constexpr (ADJ) {
                if (tb - l < s1 && lane < d) lamT[(tb - l) * d + lane] = acc;
            } else if (own) {
                const double mm = readlane_d(acc, obs_lane);
                outm = lane == l ? mm : outm;
            }
        }
        const long long t = tb - lane;
        if (!ADJ && own && lane < nb && t < s1) {
            mean[t] = y[t] + outm;
            store_var(var, t, T, qtab, n1, vbase, qinf, Rnew, rnew_per_step);
        }
    }
    if (chunk == 0 && lane < d) lam_out[lane] = zb[lane];      // lam at the head's end: the head's backward pass runs on the host
}

// ---- d <= 47: FOUR chunks per wave, no LDS.  A row of sixteen lanes holds one chunk's state in NB registers (lane p: components p, p + 16, ...; NB = 1
// for d <= 15, 2 for d <= 31, 3 for d <= 47) and the NB matching rows of the matrix, 16 NB columns each; component j reaches the row's lanes as the DPP
// operand of the multiply-add itself (v_fmac_f64_dpp row_newbcast:j), and so does the step's observation out of the row's block of sixteen.  NB = 2: 66
// multiply-adds per step and wave for four chunks (the LDS form: 32 and 16 broadcast reads for one); NB = 3: 146 against 64 and 32, 144 doubles of rows,
// a fifth of them in accumulation registers (v_accvgpr reads ahead of their multiply-adds).  The table is the LDS kernels' (DP = 32; NB = 3: DP = 64).
// (measured: 8-9 cycles per v_fmac_f64_dpp at one wave per SIMD, four accumulator chains or two alike -- 0.187 ms at d = 28, T = 1e6; two 32-bit
//  DPP moves and two plain multiply-adds per component instead run at the full issue rate and come to 0.208 ms; the LDS form 0.36 ms)
template <int J>
__device__ __forceinline__ void fmac_bc(double& acc, double src, double mul) {      // acc += (lane J of the row's src) * mul
    asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(mul), "n"(J));
}
// (a DPP operand must not be read within two cycles of the VALU write of its register, nor within five of a write to EXEC: the recogniser that
//  spaces such pairs does not look into inline assembly.  Every register a step's multiply-adds read through DPP passes here first)
__device__ __forceinline__ void dpp_settle(double& a, double& b) { asm volatile("s_nop 4" : "+v"(a), "+v"(b) : : "memory"); }
__device__ __forceinline__ void dpp_settle(double& a, double& b, double& c) { asm volatile("s_nop 4" : "+v"(a), "+v"(b), "+v"(c) : : "memory"); }
__device__ __forceinline__ void dpp_settle(double& a, double& b, double& c, double& e) { asm volatile("s_nop 4" : "+v"(a), "+v"(b), "+v"(c), "+v"(e) : : "memory"); }
__device__ __forceinline__ void dpp_settle(double& a, double& b, double& c, double& e, double& f) {
    asm volatile("s_nop 4" : "+v"(a), "+v"(b), "+v"(c), "+v"(e), "+v"(f) : : "memory");
}
template <int NB, int... Os, class... X>
__device__ __forceinline__ void dpp_settle(double (&z)[NB], std::integer_sequence<int, Os...>, X&... x) {
    dpp_settle(z[Os]..., x...);
}
struct Acc4 {
    double v[4];
    __device__ __forceinline__ double sum() const { return (v[0] + v[1]) + (v[2] + v[3]); }
};
template <int OFF, int W, int... Js>
__device__ __forceinline__ void dot16(Acc4& a, double z, const double (&phi)[W], std::integer_sequence<int, Js...>) {
    (fmac_bc<Js>(a.v[Js % 4], z, phi[OFF + Js]), ...);
}
template <int OFF, int W, int... Js>      // two outputs of the lane against the same sixteen components, their chains interleaved (eight independent accumulators)
__device__ __forceinline__ void dot16ab(Acc4& a, Acc4& b, double z, const double (&pA)[W], const double (&pB)[W], std::integer_sequence<int, Js...>) {
    ((fmac_bc<Js>(a.v[Js % 4], z, pA[OFF + Js]), fmac_bc<Js>(b.v[Js % 4], z, pB[OFF + Js])), ...);
}
typedef std::make_integer_sequence<int, 16> Seq16;
// n[o] = (output o's accumulators a[o], which hold the step's inputs) + P[o] . z for the lane's NB outputs -- the two outputs of NB = 2 interleaved, the
// three of NB = 3 one after the other
template <int NB>
__device__ __forceinline__ void rows_dot(double (&n)[NB], Acc4 (&a)[NB], const double (&z)[NB], const double (&P)[NB][16 * NB]) {
    if constexpr (NB == 2) {
        dot16ab<0>(a[0], a[1], z[0], P[0], P[1], Seq16{});
        dot16ab<16>(a[0], a[1], z[1], P[0], P[1], Seq16{});
    } else {
#pragma unroll
        for (int o = 0; o < NB; ++o) {
            dot16<0>(a[o], z[0], P[o], Seq16{});
            if constexpr (NB == 3) {
                dot16<16>(a[o], z[1], P[o], Seq16{});
                dot16<32>(a[o], z[2], P[o], Seq16{});
            }
        }
    }
#pragma unroll
    for (int o = 0; o < NB; ++o) n[o] = a[o].sum();
}
template <int NB>
__device__ __forceinline__ double pick(const double (&n)[NB], int o) {      // n[o], o wave-uniform
    const double n0 = n[0], n1 = n[NB >= 2 ? 1 : 0], n2 = n[NB - 1];      // (locals: the choice is made by selects)
    return o == 0 ? n0 : (o == 1 ? n1 : n2);
}

struct RowGeom {      // per lane, the same within a row
    long long chunk, s0, s1, w;      // own steps [s0, s1); w: where the recursion starts (forward: w <= s0, upwards; backward: w >= s1, downwards from w - 1)
    bool valid, from_head;           // from_head (forward): the recursion starts at the head's end from the head's own end state, not `halo` steps early from zero
};
template <bool FWD>
__device__ __forceinline__ RowGeom row_geom(long long T, long long t_head, long long chunk_len, long long halo, long long chunks) {
    RowGeom g;
    g.chunk = (long long)blockIdx.x * 4 + (threadIdx.x >> 4);
    g.valid = g.chunk < chunks;
    g.s0 = t_head + g.chunk * chunk_len;
    g.s1 = g.s0 + chunk_len;
    if (g.s1 > T) g.s1 = T;
    g.from_head = FWD && g.s0 - halo <= t_head;
    if (FWD) {
        g.w = g.from_head ? t_head : g.s0 - halo;
    } else {
        g.w = g.s1 + halo;
        if (g.w > T) g.w = T;
    }
    if (!g.valid) g.s0 = g.s1 = g.w = T;
    return g;
}
__device__ __forceinline__ long long longest_row(long long len) {      // the largest of the four rows' number of steps (wave-uniform)
    long long nmax = 0;
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
        const int lo = __builtin_amdgcn_readlane((int)(len & 0xffffffffll), 16 * r4), hi = __builtin_amdgcn_readlane((int)(len >> 32), 16 * r4);
        const long long v = ((long long)hi << 32) | (unsigned)lo;
        nmax = v > nmax ? v : nmax;
    }
    return nmax;
}
template <int NB>
constexpr int kTabDP = NB <= 2 ? 32 : 64;      // the rows of the matrix in the table of a model with NB components per lane (the LDS kernels' DP)
// the lane's NB rows of the table's matrix and their input gains (the table's row behind the matrix)
template <int NB>
__device__ __forceinline__ void load_rows(const double* __restrict__ tab, int p, double (&P)[NB][16 * NB], double (&kin)[NB]) {
    constexpr int DP = kTabDP<NB>;
#pragma unroll
    for (int o = 0; o < NB; ++o) {
#pragma unroll
        for (int j = 0; j < 16 * NB; ++j) P[o][j] = tab[(size_t)j * 64 + 16 * o + p];
        kin[o] = tab[(size_t)DP * 64 + 16 * o + p];
    }
}

template <int L, bool KEEP, int NB>
__device__ __forceinline__ void fwd_step4(double& yv, double (&z)[NB], const double (&P)[NB][16 * NB], const double (&kin)[NB], const double (&cin)[NB], long long t,
                                          const RowGeom& g, int obs_o, bool is_obs, double& ssq, double* __restrict__ rout, double* __restrict__ mout, int d, int p) {
    dpp_settle(z, std::make_integer_sequence<int, NB>{}, yv);
    Acc4 a[NB];
#pragma unroll
    for (int o = 0; o < NB; ++o) {
        a[o] = Acc4{{cin[o], 0.0, 0.0, 0.0}};
        fmac_bc<L>(a[o].v[3], yv, kin[o]);
    }
    double n[NB];
    rows_dot<NB>(n, a, z, P);
    const bool live = t < g.s1;
#pragma unroll
    for (int o = 0; o < NB; ++o) z[o] = live ? n[o] : z[o];
    const bool own = live && t >= g.s0;
    double rr = pick<NB>(n, obs_o);
    rr = own ? rr : 0.0;
    ssq = fma(rr, rr, ssq);
    if (KEEP) {
        if (is_obs && own) rout[t] = rr;
    }
    if (mout != nullptr) {      // (_filter: the filtered mean of the chunk's own steps -- wave-uniform test)
#pragma unroll
        for (int o = 0; o < NB; ++o)
            if (own && 16 * o + p < d) mout[t * d + 16 * o + p] = n[o];
    }
}
template <bool KEEP, int NB, int... Ls>
__device__ __forceinline__ void fwd_block4(double& yv, double (&z)[NB], const double (&P)[NB][16 * NB], const double (&kin)[NB], const double (&cin)[NB], long long t0,
                                           const RowGeom& g, int obs_o, bool is_obs, double& ssq, double* __restrict__ rout, double* __restrict__ mout, int d, int p,
                                           std::integer_sequence<int, Ls...>) {
    (fwd_step4<Ls, KEEP, NB>(yv, z, P, kin, cin, t0 + Ls, g, obs_o, is_obs, ssq, rout, mout, d, p), ...);
}

template <bool KEEP, int NB>
__global__ __launch_bounds__(64) void k_wide_lml4(const double* __restrict__ tab, const double* __restrict__ y, double hh, long long T, long long t_head, long long chunk_len,
                                                   long long halo, long long chunks, int d, ZArg z0, double* __restrict__ part, double* __restrict__ rout,
                                                   const double* __restrict__ ht, double* __restrict__ mout) {
    auto obs = [&](long long t) { return y[t] - (ht != nullptr ? ht[t] : 0.0); };      // (see k_wide_lml)
    const int p = threadIdx.x & 15;
    const RowGeom g = row_geom<true>(T, t_head, chunk_len, halo, chunks);
    double P[NB][16 * NB], kin[NB], cin[NB], z[NB];
    load_rows<NB>(tab, p, P, kin);
#pragma unroll
    for (int o = 0; o < NB; ++o) {
        cin[o] = tab[(size_t)(kTabDP<NB> + 1) * 64 + 16 * o + p] - kin[o] * hh;      // (u = y - hh folded into the constant)
        z[o] = (g.valid && g.from_head) ? z0.z[16 * o + p] : 0.0;
    }
    const int obs_o = d >> 4;      // the observer (component d) is output obs_o of lane d & 15
    const bool is_obs = p == (d & 15);
    const long long nmax = longest_row(g.s1 - g.w);
    double ssq = 0.0;
    double yn = (g.w + p < g.s1) ? obs(g.w + p) : 0.0;
    for (long long kb = 0; kb < nmax; kb += 16) {
        double yv = yn;
        yn = (g.w + kb + 16 + p < g.s1) ? obs(g.w + kb + 16 + p) : 0.0;      // (the next block: on its way while this one runs)
        fwd_block4<KEEP, NB>(yv, z, P, kin, cin, g.w + kb, g, obs_o, is_obs, ssq, rout, mout, d, p, Seq16{});
    }
    if (is_obs && g.valid) part[g.chunk] = ssq;
}

template <int L, int NB, bool ADJ>
__device__ __forceinline__ void bwd_step4(double& rv, double& yv, double (&z)[NB], const double (&P)[NB][16 * NB], const double (&kin)[NB], const double (&yin)[NB], long long t,
                                          const RowGeom& g, int obs_o, bool is_obs, double* __restrict__ mean, double* __restrict__ lamT, int d, int p) {
    dpp_settle(z, std::make_integer_sequence<int, NB>{}, rv, yv);
    Acc4 a[NB];
#pragma unroll
    for (int o = 0; o < NB; ++o) {
        a[o] = Acc4{{0.0, 0.0, 0.0, 0.0}};
        fmac_bc<L>(a[o].v[3], rv, kin[o]);
        fmac_bc<L>(a[o].v[2], yv, yin[o]);      // (1 at the observer: its sum is the step's mean; its slot of the state multiplies a zero column)
    }
    double n[NB];
    rows_dot<NB>(n, a, z, P);
    const bool live = t >= g.s0;
#pragma unroll
    for (int o = 0; o < NB; ++o) z[o] = live ? n[o] : z[o];
    if constexpr (ADJ) {      // (lam_t of the row's own steps: see k_wide_bwd)
        if (live && t < g.s1) {
#pragma unroll
            for (int o = 0; o < NB; ++o)
                if (16 * o + p < d) lamT[t * d + 16 * o + p] = n[o];
        }
    } else {
        if (is_obs && live && t < g.s1) mean[t] = pick<NB>(n, obs_o);
    }
}
template <int NB, bool ADJ, int... Ls>
__device__ __forceinline__ void bwd_block4(double& rv, double& yv, double (&z)[NB], const double (&P)[NB][16 * NB], const double (&kin)[NB], const double (&yin)[NB], long long t0,
                                           const RowGeom& g, int obs_o, bool is_obs, double* __restrict__ mean, double* __restrict__ lamT, int d, int p,
                                           std::integer_sequence<int, Ls...>) {
    (bwd_step4<Ls, NB, ADJ>(rv, yv, z, P, kin, yin, t0 - Ls, g, obs_o, is_obs, mean, lamT, d, p), ...);
}

template <int NB, bool ADJ = false>
__global__ __launch_bounds__(64) void k_wide_bwd4(const double* __restrict__ tab, const double* __restrict__ y, const double* __restrict__ r, const double* __restrict__ Rnew,
                                                   int rnew_per_step, const double* __restrict__ qtab, long long n1, double vbase, double qinf, long long T, long long t_head,
                                                   long long chunk_len, long long halo, long long chunks, int d, double* __restrict__ mean, double* __restrict__ var,
                                                   double* __restrict__ lam_out, double* __restrict__ lamT) {
    const int p = threadIdx.x & 15;
    const RowGeom g = row_geom<false>(T, t_head, chunk_len, halo, chunks);
    const int obs_o = d >> 4;
    const bool is_obs = p == (d & 15);
    double P[NB][16 * NB], kin[NB], yin[NB], z[NB];
    load_rows<NB>(tab, p, P, kin);
#pragma unroll
    for (int o = 0; o < NB; ++o) {
        yin[o] = (is_obs && o == obs_o) ? 1.0 : 0.0;
        z[o] = 0.0;
    }
    const long long nmax = longest_row(g.w - g.s0);
    const long long top = g.w - 1;      // the row's first step
    double rn = (top - p >= g.s0) ? r[top - p] : 0.0;
    for (long long kb = 0; kb < nmax; kb += 16) {      // the block holds the steps top - kb, top - kb - 1, ..., one per lane of the row
        double rv = rn;
        const long long tl = top - kb - p;
        rn = (tl - 16 >= g.s0) ? r[tl - 16] : 0.0;
        const bool mine = tl >= g.s0 && tl < g.s1;
        double yv = (!ADJ && mine) ? y[tl] : 0.0;
        bwd_block4<NB, ADJ>(rv, yv, z, P, kin, yin, top - kb, g, obs_o, is_obs, mean, lamT, d, p, Seq16{});
        if (!ADJ && mine) store_var(var, tl, T, qtab, n1, vbase, qinf, Rnew, rnew_per_step);
    }
    if (g.valid && g.chunk == 0) {      // lam at the head's end: the head's backward pass runs on the host
#pragma unroll
        for (int o = 0; o < NB; ++o)
            if (16 * o + p < d) lam_out[16 * o + p] = z[o];
    }
}

// ---- rand (lgssm.jl:65-91 with the draws supplied): x_t = A x_(t-1) + a + U' eps_t (U = chol(Q + 1e-9 I), lgc.jl:84-87), y_t = h . x_t + hh + sqrt(R) e_t
// (lgc.jl:241-243).  The same shape as k_wide_lml -- a lane per component, the state round an LDS line -- with a second line for the step's draws; the
// open loop A forgets a state as the closed loop does, so a chunk warms up `halo` steps early from zero ON THE SAME DRAWS.  tab: [2 DP + 1][64] -- columns
// of the lanes' rows of A (observer, lane d: g = A' h), of U' (observer: U h), then the constants (a_i; observer: h . a + hh).
template <int DP>
__global__ __launch_bounds__(64) void k_wide_rand(const double* __restrict__ tab, const double* __restrict__ eps_t, const double* __restrict__ eps_e, double sqrtR,
                                                   long long T, long long chunk_len, long long halo, int obs_lane, int d, ZArg x0, double* __restrict__ y_out) {
    __shared__ __attribute__((aligned(16))) double zb[64];
    __shared__ __attribute__((aligned(16))) double eb[4][64];
    const int lane = threadIdx.x;
    const long long chunk = blockIdx.x;
    const long long s0 = chunk * chunk_len;
    long long s1 = s0 + chunk_len;
    if (s1 > T) s1 = T;
    const bool from_start = s0 - halo <= 0;
    const long long w0 = from_start ? 0 : s0 - halo;
    double pa[DP], pu[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        pa[j] = tab[(size_t)j * 64 + lane];
        pu[j] = tab[(size_t)(DP + j) * 64 + lane];
    }
    const double cin = tab[(size_t)(2 * DP) * 64 + lane];
    zb[lane] = from_start ? x0.z[lane] : 0.0;
    lds_sync();
    auto draw = [&](long long t) { return (lane < d && t < s1) ? eps_t[t * d + lane] : 0.0; };
    // the draws of four steps ahead are on their way while a step runs
    double e0 = draw(w0), e1 = draw(w0 + 1), e2 = draw(w0 + 2), e3 = draw(w0 + 3);
    double outy = 0.0;
    for (long long t4 = w0; t4 < s1; t4 += 4) {
        eb[0][lane] = e0;
        eb[1][lane] = e1;
        eb[2][lane] = e2;
        eb[3][lane] = e3;
        e0 = draw(t4 + 4);
        e1 = draw(t4 + 5);
        e2 = draw(t4 + 6);
        e3 = draw(t4 + 7);
        lds_sync();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long t = t4 + k;
            if (t < s1) {      // (wave-uniform)
                double a0 = cin, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
                for (int j = 0; j < DP; j += 4) {
                    const v2d q0 = *reinterpret_cast<const v2d*>(&zb[j]), q1 = *reinterpret_cast<const v2d*>(&zb[j + 2]);
                    const v2d r0 = *reinterpret_cast<const v2d*>(&eb[k][j]), r1 = *reinterpret_cast<const v2d*>(&eb[k][j + 2]);
                    a0 = fma(pa[j], q0.x, a0);
                    a1 = fma(pa[j + 1], q0.y, a1);
                    a2 = fma(pa[j + 2], q1.x, a2);
                    a3 = fma(pa[j + 3], q1.y, a3);
                    a0 = fma(pu[j], r0.x, a0);
                    a1 = fma(pu[j + 1], r0.y, a1);
                    a2 = fma(pu[j + 2], r1.x, a2);
                    a3 = fma(pu[j + 3], r1.y, a3);
                }
                const double acc = (a0 + a1) + (a2 + a3);
                lds_sync();
                zb[lane] = acc;
                lds_sync();
                if (t >= s0) {
                    const double yy = readlane_d(acc, obs_lane);
                    outy = lane == (int)((t - s0) & 63) ? yy : outy;
                    if (((t - s0) & 63) == 63 || t == s1 - 1) {      // (a block of up to 64 emissions: one coalesced store)
                        const long long tb = t - ((t - s0) & 63), tl = tb + lane;
                        if (tl <= t) y_out[tl] = outy + sqrtR * eps_e[tl];
                    }
                }
            }
        }
    }
}

// ---- rand of posterior(model, y) with the draws supplied (lgssm.jl:65-91 on the Reverse model of :193-238), behind the head, in the deviation from the
// filtered mean dl_t = x_t - m_t: dl_(t-1) = G dl_t + (G K) r_t + U' eps_t, y*_t = y_t - (R / S) r_t + h . dl_t + sqrt(Rnew_t) e_t -- r the forward kernel's
// innovations, G and U = chol(L + 1e-9 I).U of invert_dynamics at the settled covariance.  k_wide_rand's shape run backward in time: a lane per component,
// the state round an LDS line, a second line for the step's draws (four steps ahead on their way), the innovations a block of 64 ahead in a register.  G
// forgets a state as the closed loop does, so a chunk starts `halo` steps behind its end from dl = 0 ON THE SAME STREAMS; the chunk that reaches the
// series' end starts from the drawn dl_(T-1).  tab: [2 DP + 1][64] -- columns of the lanes' rows of G (observer, lane d: h, so that its sum is h . dl_t
// of the state the step READS), of U' (observer: zero), then the gains (G K)_i on r_t (observer: zero).  Emissions leave in coalesced blocks of 64.
template <int DP>
__global__ __launch_bounds__(64) void k_wide_post_rand(const double* __restrict__ tab, const double* __restrict__ y, const double* __restrict__ r,
                                                        const double* __restrict__ eps_t, const double* __restrict__ eps_e, const double* __restrict__ Rnew,
                                                        int rnew_per_step, double rs, long long T, long long t_head, long long chunk_len, long long halo, int obs_lane,
                                                        int d, ZArg xT, double* __restrict__ y_out, double* __restrict__ x_out) {
    __shared__ __attribute__((aligned(16))) double zb[64];
    __shared__ __attribute__((aligned(16))) double eb[4][64];
    const int lane = threadIdx.x;
    const long long chunk = blockIdx.x;
    const long long s0 = t_head + chunk * chunk_len;
    long long s1 = s0 + chunk_len;
    if (s1 > T) s1 = T;
    const bool from_end = s1 + halo >= T;
    const long long w1 = from_end ? T : s1 + halo;
    double pg[DP], pu[DP];
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        pg[j] = tab[(size_t)j * 64 + lane];
        pu[j] = tab[(size_t)(DP + j) * 64 + lane];
    }
    const double kin = tab[(size_t)(2 * DP) * 64 + lane];
    zb[lane] = from_end ? xT.z[lane] : 0.0;
    lds_sync();
    auto draw = [&](long long t) { return (lane < d && t >= s0) ? eps_t[t * d + lane] : 0.0; };
    double e0 = draw(w1 - 1), e1 = draw(w1 - 2), e2 = draw(w1 - 3), e3 = draw(w1 - 4);
    double rn = (w1 - 1 - lane >= s0) ? r[w1 - 1 - lane] : 0.0;
    for (long long tb = w1 - 1; tb >= s0; tb -= 64) {      // the block holds the steps tb, tb - 1, ..., one per lane
        const double rv = rn;
        rn = (tb - 64 - lane >= s0) ? r[tb - 64 - lane] : 0.0;
        const int nb = (int)((tb - s0 + 1 < 64) ? (tb - s0 + 1) : 64);
        const bool own = tb - 63 < s1;      // (some step of the block is the chunk's own)
        double outy = 0.0;
        for (int l4 = 0; l4 < nb; l4 += 4) {
            eb[0][lane] = e0;
            eb[1][lane] = e1;
            eb[2][lane] = e2;
            eb[3][lane] = e3;
            const long long tn = tb - l4 - 4;
            e0 = draw(tn);
            e1 = draw(tn - 1);
            e2 = draw(tn - 2);
            e3 = draw(tn - 3);
            lds_sync();
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int l = l4 + k;
                if (l < nb) {      // (wave-uniform)
                    double a0 = kin * readlane_d(rv, l), a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
                    for (int j = 0; j < DP; j += 4) {
                        const v2d q0 = *reinterpret_cast<const v2d*>(&zb[j]), q1 = *reinterpret_cast<const v2d*>(&zb[j + 2]);
                        const v2d r0 = *reinterpret_cast<const v2d*>(&eb[k][j]), r1 = *reinterpret_cast<const v2d*>(&eb[k][j + 2]);
                        a0 = fma(pg[j], q0.x, a0);
                        a1 = fma(pg[j + 1], q0.y, a1);
                        a2 = fma(pg[j + 2], q1.x, a2);
                        a3 = fma(pg[j + 3], q1.y, a3);
                        a0 = fma(pu[j], r0.x, a0);
                        a1 = fma(pu[j + 1], r0.y, a1);
                        a2 = fma(pu[j + 2], r1.x, a2);
                        a3 = fma(pu[j + 3], r1.y, a3);
                    }
                    const double acc = (a0 + a1) + (a2 + a3);
                    lds_sync();      // (every lane has read the old state)
                    zb[lane] = acc;
                    lds_sync();
                    if (own) {
                        const double hx = readlane_d(acc, obs_lane);
                        outy = lane == l ? hx : outy;
                    }
                }
            }
        }
        const long long t = tb - lane;
        if (own && lane < nb && t < s1) y_out[t] = (y[t] - rs * rv) + outy + sqrt(rnew_per_step ? Rnew[t] : Rnew[0]) * eps_e[t];
    }
    if (chunk == 0 && lane < d) x_out[lane] = zb[lane];      // dl at the head's end: the head's steps run on the host
}

// _filter's covariances behind the head: the settled one (block n0 - 1, which the head's copy has just put there) into every later block
__global__ __launch_bounds__(256) void k_wide_fill_cov(double* __restrict__ P, long long n0, long long T, int dd) {
    const double* __restrict__ src = P + (n0 - 1) * dd;
    const long long n = (T - n0) * dd;
    double* __restrict__ dst = P + n0 * dd;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) dst[i] = src[i % dd];
}

// ---- the adjoint pass's sums: G = sum_t u_t w_t' over the steps behind the head, u_t = (lam_(t+1), r_t, 1), w_t = (m_(t-1), r_t, 1) -- lam from the
// ADJ backward kernels (lamT [T][d], lam_T = 0), m the filtered means from the forward kernel (m [T][d], row n0 - 1 the head's end state), r its
// innovations.  A tall-skinny split-K product on v_mfma_f64_16x16x4_f64: a wave takes `span` consecutive steps, four per MFMA (k = lane >> 4 the
// step, lane & 15 the component within a 16-wide tile), and keeps the (16 NT)^2 sums in NT^2 accumulator tiles (C/D of the f64 form:
// row = (lane >> 4) + 4 reg, col = lane & 15); its partial goes to part [wave][16 NT][16 NT], summed in wave order by k_wide_gram_sum.
typedef double d4v __attribute__((ext_vector_type(4)));
template <int NT>
__global__ __launch_bounds__(256) void k_wide_gram(const double* __restrict__ lamT, const double* __restrict__ m, const double* __restrict__ r, long long t_head,
                                                   long long T, long long span, int d, double* __restrict__ part) {
    constexpr int NG = 16 * NT;
    const int lane = threadIdx.x & 63, kq = lane >> 4, c15 = lane & 15;
    const long long w = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long long a0 = t_head + w * span;
    long long a1 = a0 + span;
    if (a1 > T) a1 = T;
    d4v acc[NT][NT];
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < NT; ++J) acc[I][J] = d4v{0.0, 0.0, 0.0, 0.0};
    for (long long tb = a0; tb < a1; tb += 4) {
        const long long t = tb + kq;
        const bool in = t < a1;
        const double rt = in ? r[t] : 0.0;
        double u[NT], v[NT];
#pragma unroll
        for (int I = 0; I < NT; ++I) {
            const int c = 16 * I + c15;
            const double tail = c == d ? rt : (c == d + 1 ? 1.0 : 0.0);
            u[I] = !in ? 0.0 : (c < d ? (t + 1 < T ? lamT[(t + 1) * d + c] : 0.0) : tail);
            v[I] = !in ? 0.0 : (c < d ? m[(t - 1) * d + c] : tail);
        }
#pragma unroll
        for (int I = 0; I < NT; ++I)
#pragma unroll
            for (int J = 0; J < NT; ++J) acc[I][J] = __builtin_amdgcn_mfma_f64_16x16x4f64(u[I], v[J], acc[I][J], 0, 0, 0);
    }
    double* out = part + w * (NG * NG);
#pragma unroll
    for (int I = 0; I < NT; ++I)
#pragma unroll
        for (int J = 0; J < NT; ++J)
#pragma unroll
            for (int q = 0; q < 4; ++q) out[(16 * I + kq + 4 * q) * NG + 16 * J + c15] = acc[I][J][q];
}
// G [ng2] = sum over the waves' partials in wave order: 64 entries per block, its four waves a quarter of the partials each, combined in a fixed order
__global__ __launch_bounds__(256) void k_wide_gram_sum(const double* __restrict__ part, long long nw, int ng2, double* __restrict__ G) {
    __shared__ double red[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + lane;
    const long long q = (nw + 3) / 4, w0 = wv * q, w1 = w0 + q < nw ? w0 + q : nw;
    double s = 0.0;
    if (e < ng2) {
#pragma unroll 8
        for (long long w = w0; w < w1; ++w) s += part[w * ng2 + e];
    }
    red[wv][lane] = s;
    __syncthreads();
    if (wv == 0 && e < ng2) G[e] = (red[0][lane] + red[1][lane]) + (red[2][lane] + red[3][lane]);
}

// ---- host: small dense linear algebra, row-major ---------------------------------------------------------------------------------------
void matmul(int d, const double* X, const double* Y, double* Z) {      // Z = X Y
    for (int i = 0; i < d; ++i) {
        double* zi = Z + (size_t)i * d;
        for (int j = 0; j < d; ++j) zi[j] = 0.0;
        for (int k = 0; k < d; ++k) {
            const double x = X[(size_t)i * d + k];
            const double* yk = Y + (size_t)k * d;
            for (int j = 0; j < d; ++j) zi[j] += x * yk[j];
        }
    }
}
double norm_inf(int d, const double* X) {
    double n = 0.0;
    for (int i = 0; i < d; ++i) {
        double s = 0.0;
        for (int j = 0; j < d; ++j) s += std::fabs(X[(size_t)i * d + j]);
        n = std::max(n, s);
    }
    return n;
}

// The kernel family that serves a planned model, chosen once by plan(): one chunk per wave round an LDS line (k_wide_lml<DP>, k_wide_bwd<DP>), or four chunks
// per wave with NB components per lane (k_wide_lml4<., NB>, k_wide_bwd4<NB>).  The name is what kernel_name() reports (profile labels, tests, bench.py).
enum Form { kLds32, kLds64, kDpp1, kDpp2, kDpp3 };
const char* form_name(Form f) {
    switch (f) {
        case kDpp1: return "k_wide_lml4<16>";
        case kDpp2: return "k_wide_lml4";
        case kDpp3: return "k_wide_lml4<48>";
        case kLds32: return "k_wide_lml<32>";
        default: return "k_wide_lml<64>";
    }
}
// Engine::pinned, in doubles: the head's y, Rnew, means, variances and emission offsets, lam at the head's end, the chunks' sums (TGP_WIDE_CHUNKS: 65536 at most)
namespace pin {
constexpr size_t yh = 0, Rh = yh + kHeadMax, mh = Rh + kHeadMax, vh = mh + kHeadMax, hth = vh + kHeadMax, lam = hth + kHeadMax, part = lam + 64, size = part + 65536;
}

}  // namespace

struct Engine {
    Info info{};
    bool have = false;
    std::vector<double> key;
    long long key_T = -1;
    int d = 0, dp = 0;
    std::vector<double> A, avec, hvec;      // row-major A, a, h
    double hh = 0.0, R = 0.0, g0 = 0.0, Sss = 0.0, sum_logS_head = 0.0;
    std::vector<double> x0m;
    std::vector<double> Kt, St;            // the head's gains [n0][d] and innovation variances [n0]
    std::vector<double> tab_host;          // the forward kernel's table (see k_wide_lml)
    // the posterior half of the plan (built by the first posterior call of a model)
    bool post_ready = false;
    int post_why = kOk;
    std::vector<double> tabb_host;         // the backward kernel's table (see k_wide_bwd)
    std::vector<double> qtab;              // partial sums of the variance's quadratic form at the series' end [n1 + 1]
    std::vector<double> headvar;           // (S_t - R) R / S_t - gw_t' Lam_(t+1) gw_t for the head's steps [n0]
    double vbase = 0.0, qinf = 0.0;
    double* dev = nullptr;                 // device: forward table | backward table | qtab
    size_t dev_cap = 0;
    bool dev_current = false, dev_post_current = false;
    double* rbuf = nullptr;                // device: the innovations of the steps behind the head [T]
    size_t rbuf_cap = 0;
    double* pinned = nullptr;              // (laid out by pin::)
    std::vector<double> head_r, head_m;
    Form form = kLds32;
    std::vector<double> Pf_head;          // the head's filtered covariances [n0][d d] (row-major = column-major: symmetric), for _filter; empty: too large
    double* rand_dev = nullptr;           // device: k_wide_rand's table
    size_t rand_cap = 0;
    // the adjoint pass (built by its first call of a planned model): the backward table of the ADJ kernels, the per-step scratch of the pass
    bool adj_ready = false;
    int adj_halo = -1;                     // -1: Psi does not forget within 2^20 steps
    std::vector<double> taba_host;         // [DP + 1][64]: rows of Psi, gains h / S (no observer)
    double *adj_dev = nullptr, *adj_pin = nullptr;      // device: forward table | backward table | G; pinned: G | the head's end state
    double *mbuf = nullptr, *lbuf = nullptr, *gpart = nullptr;      // device: m [T][d], lam [T][d], partial sums of G
    size_t mbuf_cap = 0, lbuf_cap = 0, gpart_cap = 0;
    // the draw half of the plan (built by the first posterior draw of a model)
    bool draw_ready = false;
    int draw_why = kOk;
    std::vector<double> tabd_host;         // k_wide_post_rand's table
    std::vector<double> Gd, Ld, Ud;        // [n0 + 1][d d] row-major: G_t, L_t, chol(L_t + 1e-9 I).U of the head's steps, entry n0 the settled step's
    std::vector<double> Uend;              // chol(P_(T-1) + 1e-12 I).U
    double *draw_dev = nullptr, *draw_pin = nullptr;      // device: forward table | draw table; pinned: the head's draws [n0][d], e [n0], outputs [n0], dl [64]
    size_t draw_pin_cap = 0;
    bool draw_dev_current = false;
};

namespace {
bool dpp_enabled() {      // TGP_WIDE_DPP=0: the LDS kernels for every d (A/B runs)
    static const bool on = [] {
        const char* sv = std::getenv("TGP_WIDE_DPP");
        return !(sv && sv[0] == '0');
    }();
    return on;
}
}  // namespace
Engine* create() { return new Engine(); }
void destroy(Engine* e) {
    if (!e) return;
    if (e->dev) (void)tgp_alloc::dev_free(e->dev);
    if (e->rbuf) (void)tgp_alloc::dev_free(e->rbuf);
    if (e->rand_dev) (void)tgp_alloc::dev_free(e->rand_dev);
    if (e->pinned) (void)tgp_alloc::host_free(e->pinned);
    for (double* p : {e->adj_dev, e->mbuf, e->lbuf, e->gpart, e->draw_dev})
        if (p) (void)tgp_alloc::dev_free(p);
    if (e->adj_pin) (void)tgp_alloc::host_free(e->adj_pin);
    if (e->draw_pin) (void)tgp_alloc::host_free(e->draw_pin);
    delete e;
}
const Info& last_plan(const Engine* e) { return e->info; }
const char* kernel_name(const Engine* e) { return form_name(e->form); }
void stationary(const Engine* e, double* K, double* S, double* vbase, double* qinf) {
    const int d = e->d, n0 = e->info.n0;
    if (K && n0 > 0)
        for (int i = 0; i < d; ++i) K[i] = e->Kt[(size_t)(n0 - 1) * d + i];
    if (S) *S = e->Sss;
    if (vbase) *vbase = e->vbase;
    if (qinf) *qinf = e->qinf;
}
bool filter_ready(const Engine* e) { return e->have && e->info.why == kOk && e->Pf_head.size() == (size_t)e->info.n0 * e->d * e->d; }

namespace {
template <class F>
void model_words(const ModelHost& m, F&& f) {
    const size_t d = (size_t)m.d;
    f(m.A, d * d); f(m.a, d); f(m.Q, d * d); f(m.H, d); f(&m.hh, 1); f(&m.R, 1); f(m.x0m, d); f(m.x0P, d * d);
}
bool same_model(const Engine* e, const ModelHost& m, long long T) {
    if (!e->have || e->key_T != T || e->d != m.d) return false;
    const double* k = e->key.data();
    bool same = true;
    model_words(m, [&](const double* p, size_t n) {
        same = same && std::memcmp(k, p, n * sizeof(double)) == 0;
        k += n;
    });
    return same;
}
// the smallest tested k with |M^k|_inf <= 2^-60 (squarings, then the lower bits of the exponent); -1: not within 2^20 steps
long long halo_of(int d, const std::vector<double>& M) {
    const size_t dd = (size_t)d * d;
    const double thr = std::ldexp(1.0, -60);
    std::vector<std::vector<double>> pw;
    pw.push_back(M);
    int j = 0;
    while (norm_inf(d, pw.back().data()) > thr) {
        if (j >= 20) return -1;
        std::vector<double> sq(dd);
        matmul(d, pw.back().data(), pw.back().data(), sq.data());
        pw.push_back(std::move(sq));
        ++j;
    }
    long long halo = 1LL << j;
    if (j >= 2) {
        std::vector<double> cur = pw[j - 1], cand(dd);
        long long ex = 1LL << (j - 1);
        const int bmin = std::max(0, j - 5);
        for (int b = j - 2; b >= bmin; --b) {
            matmul(d, cur.data(), pw[b].data(), cand.data());
            if (norm_inf(d, cand.data()) > thr) {
                cur = cand;
                ex += 1LL << b;
            }
        }
        halo = ex + (1LL << bmin);
    }
    return halo;
}
}  // namespace

bool plan(Engine* e, const ModelHost& m, long long T) {
    if (same_model(e, m, T)) {
        e->info.plan_ms = 0.0;
        return e->info.why == kOk;
    }
    static const bool cpu_ok = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");      // (this object's host code is built with both)
    if (!cpu_ok) {
        e->info = Info{};
        e->info.why = kAlloc;
        return false;
    }
    const auto t_begin = std::chrono::steady_clock::now();
    e->have = false;
    e->dev_current = false;
    e->post_ready = false;
    e->adj_ready = false;
    e->draw_ready = false;
    e->info = Info{};
    const int d = m.d;
    const size_t dd = (size_t)d * d;
    e->d = d;
    e->dp = d <= 31 ? 32 : 64;
    const bool dpp = d <= 47 && dpp_enabled();
    e->form = dpp ? (d <= 15 ? kDpp1 : d <= 31 ? kDpp2 : kDpp3) : (e->dp == 32 ? kLds32 : kLds64);
    e->A.assign(dd, 0.0);
    std::vector<double> Q(dd), P(dd), AP(dd), Pp(dd), Pf(dd), v(d);
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < d; ++k) {
            e->A[(size_t)i * d + k] = m.A[i + (size_t)k * d];
            Q[(size_t)i * d + k] = 0.5 * (m.Q[i + (size_t)k * d] + m.Q[k + (size_t)i * d]);
            P[(size_t)i * d + k] = 0.5 * (m.x0P[i + (size_t)k * d] + m.x0P[k + (size_t)i * d]);
        }
    e->avec.assign(m.a, m.a + d);
    e->hvec.assign(m.H, m.H + d);
    e->x0m.assign(m.x0m, m.x0m + d);
    e->hh = m.hh;
    e->R = m.R;
    const double* A = e->A.data();
    const double* h = e->hvec.data();
    auto done = [&](int why) {
        e->info.why = why;
        e->info.plan_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
        // (a plan that declined is kept as well: the next call of the same model asks no more than the memcmp)
        e->key.clear();
        model_words(m, [&](const double* p, size_t n) { e->key.insert(e->key.end(), p, p + n); });
        e->key_T = T;
        e->have = true;
        return why == kOk;
    };
    // ---- the covariance half of lgssm.jl:99-165 to its fixed point: P <- A P A' + Q; S = h' P h + R; K = P h / S; P <- P - K S K'
    e->Kt.clear();
    e->St.clear();
    e->Pf_head.clear();
    bool keep_pf = true;
    e->sum_logS_head = 0.0;
    int n0 = -1;
    double prev_chg = 1e300, rate = 0.0, prev_S = 0.0;
    for (int t = 0; t < kHeadMax; ++t) {
        matmul(d, A, P.data(), AP.data());
        double scale = 0.0;
        for (int i = 0; i < d; ++i)
            for (int j = 0; j <= i; ++j) {
                const double *x = AP.data() + (size_t)i * d, *yv = A + (size_t)j * d;
                double s = Q[(size_t)i * d + j];
                for (int k = 0; k < d; ++k) s += x[k] * yv[k];
                Pp[(size_t)i * d + j] = Pp[(size_t)j * d + i] = s;
            }
        double S = m.R;
        for (int i = 0; i < d; ++i) {
            double s = 0.0;
            for (int k = 0; k < d; ++k) s += Pp[(size_t)i * d + k] * h[k];
            v[i] = s;
            S += h[i] * s;
        }
        if (!(S > 0.0) || !std::isfinite(S)) return done(kNotPD);
        const double iS = 1.0 / S;
        double chg = 0.0;
        for (int i = 0; i < d; ++i)
            for (int j = 0; j <= i; ++j) {
                const double pf = Pp[(size_t)i * d + j] - v[i] * v[j] * iS;
                chg = std::max(chg, std::fabs(pf - P[(size_t)i * d + j]));
                scale = std::max(scale, std::fabs(pf));
                Pf[(size_t)i * d + j] = Pf[(size_t)j * d + i] = pf;
            }
        for (int i = 0; i < d; ++i) e->Kt.push_back(v[i] * iS);
        e->St.push_back(S);
        e->sum_logS_head += std::log(S);
        if (keep_pf) {
            if (e->Pf_head.size() + dd > ((size_t)64 << 20) / sizeof(double)) {      // (64 MB of head covariances at most: beyond, _filter is the dense engine's)
                keep_pf = false;
                e->Pf_head.clear();
            } else {
                e->Pf_head.insert(e->Pf_head.end(), Pf.begin(), Pf.end());
            }
        }
        P.swap(Pf);
        // the contraction rate, while the changes are still well above rounding: "no longer moves" bounds the DISTANCE to the fixed point by
        // (last change) / (1 - rate) only -- a recursion that creeps (fine spacings: rate -> 1) is not settled when its steps fall to the rounding floor
        if (chg > 1e-11 * scale && prev_chg > 1e-11 * scale && chg < prev_chg) rate = chg / prev_chg;
        // settled: the step changes nothing at all, or nothing beyond rounding -- a few ulps of the largest entry, or no longer shrinking at the rounding
        // floor -- with the fixed point within 1e-12 of it by that bound
        // (... and the innovation variance -- what the log-likelihood sees -- within 1e-13 of ITS fixed point: S can be orders of magnitude below the
        //  covariance's largest entry)
        const bool still = chg <= 4.0 * 2.220446049250313e-16 * scale || (t >= 16 && chg >= prev_chg && chg <= 1e-13 * scale);
        const double dS = std::fabs(S - prev_S);
        if (chg == 0.0 || (still && chg <= (1.0 - rate) * 1e-12 * scale && dS <= (1.0 - rate) * 1e-13 * S)) {
            n0 = t + 1;
            break;
        }
        prev_chg = chg;
        prev_S = S;
    }
    if (n0 < 0) return done(kNotSettled);
    e->info.n0 = n0;
    e->info.nhs = n0;
    e->Sss = e->St.back();
    const double* K = e->Kt.data() + (size_t)(n0 - 1) * d;
    // ---- Phi = (I - K h') A = A - K g', g = A' h; c = a - K g0, g0 = h . a
    std::vector<double> g(d, 0.0), Phi(dd);
    for (int k = 0; k < d; ++k)
        for (int j = 0; j < d; ++j) g[j] += h[k] * A[(size_t)k * d + j];
    double g0 = 0.0;
    for (int k = 0; k < d; ++k) g0 += h[k] * e->avec[k];
    e->g0 = g0;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) Phi[(size_t)i * d + j] = A[(size_t)i * d + j] - K[i] * g[j];
    const long long halo = halo_of(d, Phi);
    if (halo < 0) return done(kSlowMixing);
    e->info.halo = (int)halo;
    const long long Tb = T - n0;      // steps behind the head
    if (Tb < 64) return done(kTooShort);
    // chunks: one wave's worth of them per SIMD (4096) at least -- none shorter than 64 steps --, and more (up to 16384: the stalls of a wave's dependent
    // DPP multiply-adds are another wave's issue slots) once a chunk is still four halos long: 12 % at T = 1e7 (scripts/r06_mid_d_time.py)
    static const long long forced_chunks = [] {      // TGP_WIDE_CHUNKS=<n>: development
        const char* sv = std::getenv("TGP_WIDE_CHUNKS");
        const long long v = sv ? std::atoll(sv) : 0;
        return v >= 1 && v <= 65536 ? v : 0ll;
    }();
    long long want = std::max<long long>(kMaxChunks, std::min<long long>(4 * (long long)kMaxChunks, Tb / (4 * std::max<long long>(halo, 16))));
    if (forced_chunks) want = forced_chunks;
    long long chunks = std::min<long long>(want, Tb / 64);
    // a slowly mixing closed loop: no chunk shorter than half its warm-up (else the warm-ups are most of the work; a chunk within `halo` of the head starts
    // from the head's own end state whatever its length)
    chunks = std::max<long long>(1, std::min<long long>(chunks, Tb / std::max<long long>(64, halo / 2)));
    long long len = (Tb + chunks - 1) / chunks;
    chunks = (Tb + len - 1) / len;
    e->info.chunks = chunks;
    e->info.chunk_len = len;
    // ---- the forward kernel's table
    const int DP = e->dp;
    e->tab_host.assign((size_t)(DP + 2) * 64, 0.0);
    for (int i = 0; i < d; ++i) {
        for (int j = 0; j < d; ++j) e->tab_host[(size_t)j * 64 + i] = Phi[(size_t)i * d + j];
        e->tab_host[(size_t)DP * 64 + i] = K[i];
        e->tab_host[(size_t)(DP + 1) * 64 + i] = e->avec[i] - K[i] * g0;
    }
    for (int j = 0; j < d; ++j) e->tab_host[(size_t)j * 64 + d] = -g[j];      // the observer: r = u - g . z - g0
    e->tab_host[(size_t)DP * 64 + d] = 1.0;
    e->tab_host[(size_t)(DP + 1) * 64 + d] = -g0;
    return done(kOk);
}

namespace {
// AK = A K and Psi = (I - h K') A' = A' - h (A K)' of the step with gain Kv: the backward recursion's matrix
void back_step(const Engine* e, const double* Kv, std::vector<double>& AK, std::vector<double>& Psi) {
    const int d = e->d;
    const double *A = e->A.data(), *h = e->hvec.data();
    for (int j = 0; j < d; ++j) {
        double s = 0.0;
        for (int k = 0; k < d; ++k) s += A[(size_t)j * d + k] * Kv[k];
        AK[j] = s;
    }
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) Psi[(size_t)i * d + j] = A[(size_t)j * d + i] - h[i] * AK[j];
}
// the backward kernels' table (see k_wide_bwd): the rows of Psi, the gains h / S; gw != nullptr: the observer's row gw and gain -R / S as well
void back_table(const Engine* e, const std::vector<double>& Psi, const double* gw, std::vector<double>& tab) {
    const int d = e->d, DP = e->dp;
    const double S = e->Sss;
    tab.assign((size_t)(DP + 1) * 64, 0.0);
    for (int i = 0; i < d; ++i) {
        for (int j = 0; j < d; ++j) tab[(size_t)j * 64 + i] = Psi[(size_t)i * d + j];
        tab[(size_t)DP * 64 + i] = e->hvec[i] / S;
    }
    if (gw == nullptr) return;
    for (int j = 0; j < d; ++j) tab[(size_t)j * 64 + d] = gw[j];      // the observer: mean_t - y_t = gw . lam_(t+1) - (R / S) r_t
    tab[(size_t)DP * 64 + d] = -e->R / S;
}

// The posterior half of the plan, data-free as the rest: Psi = (I - h K') A' and gw = R A K of the stationary step, halo_back, the partial sums
// q_j = sum_(k < j) (gw' Psi^k h)^2 / S of the variance's quadratic form at the series' end (n1 of them until they no longer change), Lam_inf = the
// fixed point of Lam = h h' / S + Psi Lam Psi' by doubling, and from it the head's variances backwards through the head's own steps.
int plan_post(Engine* e, long long T) {
    const int d = e->d, n0 = e->info.n0;
    const size_t dd = (size_t)d * d;
    const double* h = e->hvec.data();
    const double R = e->R, S = e->Sss;
    std::vector<double> AK(d), Psi(dd), gw(d);
    back_step(e, e->Kt.data() + (size_t)(n0 - 1) * d, AK, Psi);
    for (int j = 0; j < d; ++j) gw[j] = R * AK[j];
    const long long hb = halo_of(d, Psi);
    if (hb < 0) return kSlowMixing;
    e->info.halo_back = (int)hb;
    // ---- the series' end: q_j
    e->qtab.assign(1, 0.0);
    {
        std::vector<double> u(h, h + d), un(d);
        double gw1 = 0.0;
        for (int j = 0; j < d; ++j) gw1 += std::fabs(gw[j]);
        double q = 0.0;
        long long n1 = -1;
        for (long long k = 0; k < kTailMax; ++k) {
            double c = 0.0, umax = 0.0;
            for (int j = 0; j < d; ++j) {
                c += gw[j] * u[j];
                umax = std::max(umax, std::fabs(u[j]));
            }
            q += c * c / S;
            e->qtab.push_back(q);
            const double bound = gw1 * umax;      // |gw' Psi^k' h| for every later k' is below this times |Psi^(k' - k)|
            if (bound * bound / S <= 1e-20 * std::max(q, 1e-300) && k >= 2) {
                n1 = k + 1;
                break;
            }
            for (int i = 0; i < d; ++i) {
                double s2 = 0.0;
                for (int j = 0; j < d; ++j) s2 += Psi[(size_t)i * d + j] * u[j];
                un[i] = s2;
            }
            u.swap(un);
        }
        if (n1 < 0) return kTailLong;
        e->info.n1 = (int)n1;
        e->qinf = q;
        if ((long long)n0 + n1 + 1 > T) return kTooShort;
    }
    e->vbase = (S - R) * R / S;
    // ---- Lam_inf by doubling: Lam <- Lam + M Lam M', M <- M^2
    std::vector<double> Lam(dd), M(Psi), T1(dd), T2(dd);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) Lam[(size_t)i * d + j] = h[i] * h[j] / S;
    for (int it = 0; it < 40; ++it) {
        if (norm_inf(d, M.data()) <= 1e-12) break;
        matmul(d, M.data(), Lam.data(), T1.data());      // T1 = M Lam
        for (int i = 0; i < d; ++i)
            for (int j = 0; j <= i; ++j) {               // Lam += T1 M'
                double s2 = 0.0;
                for (int k = 0; k < d; ++k) s2 += T1[(size_t)i * d + k] * M[(size_t)j * d + k];
                T2[(size_t)i * d + j] = T2[(size_t)j * d + i] = s2;
            }
        for (size_t i = 0; i < dd; ++i) Lam[i] += T2[i];
        matmul(d, M.data(), M.data(), T1.data());
        M.swap(T1);
    }
    // ---- the head's variances, backwards through its own steps (row n0 - 1 first: Lam_(n0) = Lam_inf)
    e->headvar.assign(n0, 0.0);
    {
        std::vector<double> AKt(d), gwt(d), Pt(dd);
        for (int t = n0 - 1; t >= 0; --t) {
            const double St = e->St[t];
            back_step(e, e->Kt.data() + (size_t)t * d, AKt, Pt);
            for (int j = 0; j < d; ++j) gwt[j] = R * AKt[j];
            double qf = 0.0;
            for (int i = 0; i < d; ++i) {
                double s2 = 0.0;
                for (int j = 0; j < d; ++j) s2 += Lam[(size_t)i * d + j] * gwt[j];
                qf += gwt[i] * s2;
            }
            e->headvar[t] = (St - R) * R / St - qf;
            if (t == 0) break;
            matmul(d, Pt.data(), Lam.data(), T1.data());
            for (int i = 0; i < d; ++i)
                for (int j = 0; j <= i; ++j) {
                    double s2 = h[i] * h[j] / St;
                    for (int k = 0; k < d; ++k) s2 += T1[(size_t)i * d + k] * Pt[(size_t)j * d + k];
                    T2[(size_t)i * d + j] = T2[(size_t)j * d + i] = s2;
                }
            Lam.swap(T2);
        }
    }
    back_table(e, Psi, gw.data(), e->tabb_host);
    return kOk;
}
}  // namespace

bool plan_posterior(Engine* e, long long T) {
    if (!e->have || e->info.why != kOk) return false;
    if (!e->post_ready) {
        const auto t_begin = std::chrono::steady_clock::now();
        e->post_why = plan_post(e, T);
        e->post_ready = true;
        e->dev_current = false;
        e->info.plan_post_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    } else {
        e->info.plan_post_ms = 0.0;
    }
    e->info.why_post = e->post_why;
    return e->post_why == kOk;
}

namespace {
// a device buffer of at least `need` bytes: the old one is freed before the larger one is asked for; on failure p == nullptr, cap == 0
hipError_t grow(double*& p, size_t& cap, size_t need) {
    if (need <= cap) return hipSuccess;
    if (p) (void)tgp_alloc::dev_free(p);
    p = nullptr;
    cap = 0;
    const hipError_t rc = tgp_alloc::dev_malloc(reinterpret_cast<void**>(&p), need);
    if (rc == hipSuccess) cap = need;
    else p = nullptr;
    return rc;
}
hipError_t pinned_ready(Engine* e) {
    return e->pinned ? hipSuccess : tgp_alloc::host_malloc(reinterpret_cast<void**>(&e->pinned), pin::size * sizeof(double), hipHostMallocDefault);
}
// The head forward: lgssm.jl:147-165 with the plan's gains, on the head's observations yh (hth: their emission offsets per step, or nullptr: the
// model's hh).  Returns the head's share of the quadratic form; z0: its end state; r_out, m_out (where asked): its innovations [n0], filtered means [n0][d].
double head_forward(const Engine* e, const double* yh, const double* hth, ZArg& z0, std::vector<double>* r_out, std::vector<double>* m_out) {
    const int d = e->d, n0 = e->info.n0;
    const double *A = e->A.data(), *h = e->hvec.data();
    double quad = 0.0;
    if (r_out) r_out->resize(n0);
    if (m_out) m_out->clear();
    std::vector<double> mcur(e->x0m), mp(d);
    for (int t = 0; t < n0; ++t) {
        double pred = hth ? hth[t] : e->hh;
        for (int i = 0; i < d; ++i) {
            double s = e->avec[i];
            const double* ai = A + (size_t)i * d;
            for (int k = 0; k < d; ++k) s += ai[k] * mcur[k];
            mp[i] = s;
            pred += h[i] * s;
        }
        const double r = yh[t] - pred;
        if (r_out) (*r_out)[t] = r;
        quad += r * r / e->St[t];
        const double* K = e->Kt.data() + (size_t)t * d;
        for (int i = 0; i < d; ++i) mcur[i] = mp[i] + K[i] * r;
        if (m_out) m_out->insert(m_out->end(), mcur.begin(), mcur.end());
    }
    for (int i = 0; i < 64; ++i) z0.z[i] = i < d ? mcur[i] : 0.0;
    return quad;
}
// logpdf from the head's quadratic form and the chunks' sums of r_t^2 (in chunk order)
double closing_lml(const Engine* e, long long T, double quad, const double* part) {
    double ssq = 0.0;
    for (long long k = 0; k < e->info.chunks; ++k) ssq += part[k];
    const double kLog2Pi = 1.8378770664093454835606594728112;
    return -0.5 * ((double)T * kLog2Pi + e->sum_logS_head + (double)(T - e->info.n0) * std::log(e->Sss) + quad + ssq / e->Sss);
}
// The forward kernel of the engine's form over the steps behind the head.  keep: the innovations go to rout (a posterior or adjoint call).
void launch_forward(const Engine* e, hipStream_t stream, bool keep, const double* tab, const double* y, long long T, const ZArg& z0, double* part, double* rout,
                    const double* ht, double* mout) {
    const int d = e->d;
    const long long n0 = e->info.n0, len = e->info.chunk_len, halo = e->info.halo, chunks = e->info.chunks;
    auto dpp = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((chunks + 3) / 4)), dim3(64), 0, stream, tab, y, e->hh, T, n0, len, halo, chunks, d, z0, part, rout, ht, mout);
    };
    auto lds = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((unsigned)chunks), dim3(64), 0, stream, tab, y, e->hh, T, n0, len, halo, d, z0, part, rout, ht, mout, d); };
    switch (e->form) {
        case kDpp1: keep ? dpp(k_wide_lml4<true, 1>) : dpp(k_wide_lml4<false, 1>); break;
        case kDpp2: keep ? dpp(k_wide_lml4<true, 2>) : dpp(k_wide_lml4<false, 2>); break;
        case kDpp3: keep ? dpp(k_wide_lml4<true, 3>) : dpp(k_wide_lml4<false, 3>); break;
        case kLds32: lds(k_wide_lml<32>); break;
        case kLds64: lds(k_wide_lml<64>); break;
    }
}
// The backward kernel of the engine's form on the innovations r.  adj: lam_t to lamT (the adjoint pass: no posterior, c is not read); else the posterior
// marginals of c with the posterior plan's tables.  lam_out: lam at the head's end.
void launch_backward(const Engine* e, hipStream_t stream, bool adj, const double* tab, const double* qtab, long long T, const double* y, const double* r, const Call& c,
                     double* lam_out, double* lamT) {
    const int d = e->d;
    const long long n0 = e->info.n0, len = e->info.chunk_len, chunks = e->info.chunks;
    const long long halo = adj ? e->adj_halo : e->info.halo_back, n1 = adj ? 0 : e->info.n1;
    const double vbase = adj ? 0.0 : e->vbase, qinf = adj ? 0.0 : e->qinf;
    const double* Rnew = adj ? nullptr : c.Rnew;
    const int per_step = adj ? 0 : c.rnew_per_step;
    double *mean = adj ? nullptr : c.mean, *var = adj ? nullptr : c.var;
    auto dpp = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)((chunks + 3) / 4)), dim3(64), 0, stream, tab, y, r, Rnew, per_step, qtab, n1, vbase, qinf, T, n0, len, halo, chunks, d, mean, var,
                           lam_out, lamT);
    };
    auto lds = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)chunks), dim3(64), 0, stream, tab, y, r, Rnew, per_step, qtab, n1, vbase, qinf, T, n0, len, halo, d, d, mean, var, lam_out, lamT);
    };
    switch (e->form) {
        case kDpp1: adj ? dpp(k_wide_bwd4<1, true>) : dpp(k_wide_bwd4<1, false>); break;
        case kDpp2: adj ? dpp(k_wide_bwd4<2, true>) : dpp(k_wide_bwd4<2, false>); break;
        case kDpp3: adj ? dpp(k_wide_bwd4<3, true>) : dpp(k_wide_bwd4<3, false>); break;
        case kLds32: adj ? lds(k_wide_bwd<32, true>) : lds(k_wide_bwd<32, false>); break;
        case kLds64: adj ? lds(k_wide_bwd<64, true>) : lds(k_wide_bwd<64, false>); break;
    }
}
}  // namespace

int run(Engine* e, hipStream_t stream, const Call& c, double* lml_out, std::string* err) {
    auto fail = [&](hipError_t rc, const char* what) {
        if (err) *err = std::string("tgp_wide: ") + what + ": " + hipGetErrorString(rc);
        return (int)rc;
    };
    const bool post = c.mean != nullptr;
    if (!e->have || e->info.why != kOk || (post && (!e->post_ready || e->post_why != kOk || !c.var || !c.Rnew))) return fail(hipErrorInvalidValue, "no plan");
    const int d = e->d, DP = e->dp, n0 = e->info.n0;
    const long long T = c.T;
    hipError_t rc = pinned_ready(e);
    if (rc != hipSuccess) return fail(rc, "pinned buffer");
    // device tables: forward | backward | qtab
    const size_t nf = e->tab_host.size(), nb = post ? e->tabb_host.size() : 0, nq = post ? e->qtab.size() : 0;
    const size_t cap_before = e->dev_cap;
    rc = grow(e->dev, e->dev_cap, (nf + (size_t)(DP + 1) * 64 + (size_t)kTailMax + 2) * sizeof(double));
    if (e->dev_cap != cap_before) e->dev_current = false;      // (a new buffer, or none)
    if (rc != hipSuccess) return fail(rc, "tables");
    double *tab_f = e->dev, *tab_b = e->dev + nf, *qtab_d = tab_b + (size_t)(DP + 1) * 64;
    if (!e->dev_current || (post && !e->dev_post_current)) {
        rc = hipMemcpyAsync(tab_f, e->tab_host.data(), nf * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc == hipSuccess && post) rc = hipMemcpyAsync(tab_b, e->tabb_host.data(), nb * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc == hipSuccess && post) rc = hipMemcpyAsync(qtab_d, e->qtab.data(), nq * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc != hipSuccess) return fail(rc, "table upload");
        e->dev_current = true;
        e->dev_post_current = post;
    }
    if (post) {
        rc = grow(e->rbuf, e->rbuf_cap, (size_t)T * sizeof(double));
        if (rc != hipSuccess) return fail(rc, "innovation buffer");
    }
    double *yh = e->pinned + pin::yh, *Rh = e->pinned + pin::Rh, *mh = e->pinned + pin::mh, *vh = e->pinned + pin::vh, *hth = e->pinned + pin::hth;
    double *lam = e->pinned + pin::lam, *part = e->pinned + pin::part;
    rc = hipMemcpyAsync(yh, c.y, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess && post) rc = hipMemcpyAsync(Rh, c.Rnew, (size_t)(c.rnew_per_step ? n0 : 1) * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess && c.h_t) rc = hipMemcpyAsync(hth, c.h_t, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc != hipSuccess) return fail(rc, "head observations");
    rc = hipStreamSynchronize(stream);
    if (rc != hipSuccess) return fail(rc, "head observations");
    ZArg z0;
    const double quad = head_forward(e, yh, c.h_t ? hth : nullptr, z0, &e->head_r, c.fm ? &e->head_m : nullptr);
    if (c.fm) {      // _filter: the head's means and covariances, the settled covariance behind them
        if (!c.fP || e->Pf_head.size() != (size_t)n0 * d * d) return fail(hipErrorInvalidValue, "filter outputs");
        rc = hipMemcpyAsync(c.fm, e->head_m.data(), (size_t)n0 * d * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc == hipSuccess) rc = hipMemcpyAsync(c.fP, e->Pf_head.data(), e->Pf_head.size() * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc != hipSuccess) return fail(rc, "head filter outputs");
        const long long nfill = (T - n0) * (long long)d * d;
        const unsigned blocks = (unsigned)std::min<long long>((nfill + 255) / 256, 16384);
        if (nfill > 0) hipLaunchKernelGGL(k_wide_fill_cov, dim3(blocks), dim3(256), 0, stream, c.fP, (long long)n0, T, d * d);
    }
    launch_forward(e, stream, post, tab_f, c.y, T, z0, part, post ? e->rbuf : nullptr, c.h_t, c.fm);
    rc = hipGetLastError();
    if (rc != hipSuccess) return fail(rc, "launch");
    if (post) {
        launch_backward(e, stream, false, tab_b, qtab_d, T, c.y, e->rbuf, c, lam, nullptr);
        rc = hipGetLastError();
        if (rc != hipSuccess) return fail(rc, "launch");
    }
    rc = hipStreamSynchronize(stream);
    if (rc != hipSuccess) return fail(rc, "kernel");
    if (post) {
        // ---- the head backward: lam_t = h r_t / S_t + Psi_t lam_(t+1), Psi_t lam = A' lam - h (A K_t) . lam; mean_t = y_t - (R / S_t) r_t + R (A K_t) . lam_(t+1)
        const double *A = e->A.data(), *h = e->hvec.data();
        std::vector<double> lcur(lam, lam + d), AKt(d), ln(d);
        for (int t = n0 - 1; t >= 0; --t) {
            const double* Kv = e->Kt.data() + (size_t)t * d;
            const double St = e->St[t], r = e->head_r[t];
            double akl = 0.0;
            for (int j = 0; j < d; ++j) {
                double s = 0.0;
                for (int k = 0; k < d; ++k) s += A[(size_t)j * d + k] * Kv[k];
                AKt[j] = s;
                akl += s * lcur[j];
            }
            mh[t] = yh[t] - (e->R / St) * r + e->R * akl;
            vh[t] = e->headvar[t] + Rh[c.rnew_per_step ? t : 0];
            for (int i = 0; i < d; ++i) {
                double s = h[i] * (r / St - akl);
                for (int k = 0; k < d; ++k) s += A[(size_t)k * d + i] * lcur[k];
                ln[i] = s;
            }
            lcur.swap(ln);
        }
        rc = hipMemcpyAsync(c.mean, mh, (size_t)n0 * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc == hipSuccess) rc = hipMemcpyAsync(c.var, vh, (size_t)n0 * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc == hipSuccess) rc = hipStreamSynchronize(stream);
        if (rc != hipSuccess) return fail(rc, "head outputs");
    }
    *lml_out = closing_lml(e, T, quad, part);
    return 0;
}

namespace {
// (G, L) = invert_dynamics (lgssm.jl:231-238) of the step whose predecessor's filtered covariance is Pprev, and U = chol(L + 1e-9 I).U (lgc.jl:84-87), all
// row-major.  The solve is against the predicted covariance + 1e-10 I, of condition up to 1e10 at d = 28: O(d^3) once per plan, so in extended precision
// (x87 long double: 64-bit significand) and rounded at the end.  false: one of the two factorisations met a pivot that is not positive.
typedef long double xreal;
bool invert_dynamics_host(int d, const double* A, const double* Q, const double* Pprev, double* G, double* L, double* U) {
    const size_t dd = (size_t)d * d;
    std::vector<xreal> AP(dd), Pp(dd), C(dd, 0.0L), X(dd), UG(dd), Lx(dd), Ux(dd, 0.0L);
    auto at = [d](int i, int j) { return (size_t)i * d + j; };
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            xreal s = 0.0L;
            for (int k = 0; k < d; ++k) s += (xreal)A[at(i, k)] * (xreal)Pprev[at(k, j)];
            AP[at(i, j)] = s;
        }
    for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
            xreal s = (xreal)Q[at(i, j)] + (i == j ? (xreal)1e-10 : 0.0L);
            for (int k = 0; k < d; ++k) s += AP[at(i, k)] * (xreal)A[at(j, k)];
            Pp[at(i, j)] = Pp[at(j, i)] = s;
        }
    for (int j = 0; j < d; ++j) {      // Pp = C C', C lower
        xreal s = Pp[at(j, j)];
        for (int k = 0; k < j; ++k) s -= C[at(j, k)] * C[at(j, k)];
        if (!(s > 0.0L)) return false;
        const xreal cj = sqrtl(s);
        C[at(j, j)] = cj;
        for (int i = j + 1; i < d; ++i) {
            xreal v = Pp[at(i, j)];
            for (int k = 0; k < j; ++k) v -= C[at(i, k)] * C[at(j, k)];
            C[at(i, j)] = v / cj;
        }
    }
    for (int c = 0; c < d; ++c) {      // X = Pp \ (A Pprev), column by column: G = X'
        for (int i = 0; i < d; ++i) {
            xreal v = AP[at(i, c)];
            for (int k = 0; k < i; ++k) v -= C[at(i, k)] * UG[at(k, c)];
            UG[at(i, c)] = v / C[at(i, i)];      // (C \ A Pprev = C' X: the factor of the term L loses)
        }
        for (int i = d - 1; i >= 0; --i) {
            xreal v = UG[at(i, c)];
            for (int k = i + 1; k < d; ++k) v -= C[at(k, i)] * X[at(k, c)];
            X[at(i, c)] = v / C[at(i, i)];
        }
    }
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) G[at(i, j)] = (double)X[at(j, i)];
    for (int i = 0; i < d; ++i)
        for (int j = 0; j <= i; ++j) {
            xreal s = 0.5L * ((xreal)Pprev[at(i, j)] + (xreal)Pprev[at(j, i)]);
            for (int k = 0; k < d; ++k) s -= UG[at(k, i)] * UG[at(k, j)];
            Lx[at(i, j)] = Lx[at(j, i)] = s;
            L[at(i, j)] = L[at(j, i)] = (double)s;
        }
    for (int j = 0; j < d; ++j)      // U' U = L + 1e-9 I, U upper
        for (int i = 0; i <= j; ++i) {
            xreal s = Lx[at(i, j)] + (i == j ? (xreal)1e-9 : 0.0L);
            for (int k = 0; k < i; ++k) s -= Ux[at(k, i)] * Ux[at(k, j)];
            if (i == j) {
                if (!(s > 0.0L)) return false;
                Ux[at(j, j)] = sqrtl(s);
            } else {
                Ux[at(i, j)] = s / Ux[at(i, i)];
            }
        }
    for (size_t i = 0; i < dd; ++i) U[i] = (double)Ux[i];
    return true;
}

// The draw half of the plan, data-free as the rest: (G_t, L_t, U_t) of the head's steps from its kept filtered covariances (step 0: the prior's), of the
// settled step behind them, halo_draw of the settled G, the factor of the last filtered covariance, the kernel's table and its chunks.
int plan_draw_build(Engine* e, long long T) {
    const int d = e->d, n0 = e->info.n0, DP = e->dp;
    const size_t dd = (size_t)d * d;
    if (e->Pf_head.size() != (size_t)n0 * dd) return kNoHeadCov;
    std::vector<double> Q(dd), P0(dd);
    {
        const double* k = e->key.data();      // (the model as handed to plan: A, a, Q, H, hh, R, x0m, x0P -- column-major blocks)
        const double *Qc = k + dd + d, *Pc = k + 2 * dd + 3 * d + 2;
        for (int i = 0; i < d; ++i)
            for (int j = 0; j < d; ++j) {
                Q[(size_t)i * d + j] = 0.5 * (Qc[i + (size_t)j * d] + Qc[j + (size_t)i * d]);
                P0[(size_t)i * d + j] = 0.5 * (Pc[i + (size_t)j * d] + Pc[j + (size_t)i * d]);
            }
    }
    e->Gd.assign((size_t)(n0 + 1) * dd, 0.0);
    e->Ld.assign((size_t)(n0 + 1) * dd, 0.0);
    e->Ud.assign((size_t)(n0 + 1) * dd, 0.0);
    for (int t = 0; t <= n0; ++t) {
        const double* Pprev = t == 0 ? P0.data() : e->Pf_head.data() + (size_t)(t - 1) * dd;
        if (!invert_dynamics_host(d, e->A.data(), Q.data(), Pprev, e->Gd.data() + (size_t)t * dd, e->Ld.data() + (size_t)t * dd, e->Ud.data() + (size_t)t * dd)) return kNotPD;
    }
    const double *G = e->Gd.data() + (size_t)n0 * dd, *U = e->Ud.data() + (size_t)n0 * dd;
    const long long halo = halo_of(d, std::vector<double>(G, G + dd));
    if (halo < 0) return kSlowMixing;
    e->info.halo_draw = (int)halo;
    // chol(P_(T-1) + 1e-12 I).U (gaussian.jl:35-43): the last filtered covariance is the settled one
    e->Uend.assign(dd, 0.0);
    {
        const double* Pe = e->Pf_head.data() + (size_t)(n0 - 1) * dd;
        std::vector<xreal> Ux(dd, 0.0L);
        for (int j = 0; j < d; ++j)
            for (int i = 0; i <= j; ++i) {
                xreal s = (xreal)Pe[(size_t)i * d + j] + (i == j ? (xreal)1e-12 : 0.0L);
                for (int k = 0; k < i; ++k) s -= Ux[(size_t)k * d + i] * Ux[(size_t)k * d + j];
                if (i == j) {
                    if (!(s > 0.0L)) return kNotPD;
                    Ux[(size_t)j * d + j] = sqrtl(s);
                } else {
                    Ux[(size_t)i * d + j] = s / Ux[(size_t)i * d + i];
                }
            }
        for (size_t i = 0; i < dd; ++i) e->Uend[i] = (double)Ux[i];
    }
    const long long Tb = T - n0;
    if (Tb < 64) return kTooShort;
    // chunks as k_wide_rand's: one wave each, none shorter than half its warm-up
    long long chunks = std::min<long long>(kMaxChunks, std::max<long long>(1, Tb / std::max<long long>(64, halo / 2)));
    const long long len = (Tb + chunks - 1) / chunks;
    chunks = (Tb + len - 1) / len;
    e->info.draw_chunks = chunks;
    e->info.draw_chunk_len = len;
    const double* K = e->Kt.data() + (size_t)(n0 - 1) * d;
    e->tabd_host.assign((size_t)(2 * DP + 1) * 64, 0.0);
    for (int i = 0; i < d; ++i) {
        double gk = 0.0;
        for (int j = 0; j < d; ++j) {
            e->tabd_host[(size_t)j * 64 + i] = G[(size_t)i * d + j];
            e->tabd_host[(size_t)(DP + j) * 64 + i] = U[(size_t)j * d + i];      // U'[i][j]
            gk += G[(size_t)i * d + j] * K[j];
        }
        e->tabd_host[(size_t)(2 * DP) * 64 + i] = gk;
    }
    for (int j = 0; j < d; ++j) e->tabd_host[(size_t)j * 64 + d] = e->hvec[j];      // the observer: h . dl_t
    return kOk;
}
}  // namespace

bool plan_draw(Engine* e, long long T) {
    if (!e->have || e->info.why != kOk) return false;
    const int halo_kept = e->info.halo_draw;
    const long long chunks_kept = e->info.draw_chunks, len_kept = e->info.draw_chunk_len;
    if (!e->draw_ready) {
        const auto t_begin = std::chrono::steady_clock::now();
        e->draw_why = plan_draw_build(e, T);
        e->draw_ready = true;
        e->draw_dev_current = false;
        e->info.plan_draw_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
    } else {
        e->info.plan_draw_ms = 0.0;
        e->info.halo_draw = halo_kept;
        e->info.draw_chunks = chunks_kept;
        e->info.draw_chunk_len = len_kept;
    }
    e->info.why_draw = e->draw_why;
    return e->draw_why == kOk;
}
void draw_stationary(const Engine* e, double* G, double* L, double* U) {
    const size_t dd = (size_t)e->d * e->d, off = (size_t)e->info.n0 * dd;
    if (!e->draw_ready || e->draw_why != kOk) return;
    if (G) std::memcpy(G, e->Gd.data() + off, dd * sizeof(double));
    if (L) std::memcpy(L, e->Ld.data() + off, dd * sizeof(double));
    if (U) std::memcpy(U, e->Ud.data() + off, dd * sizeof(double));
}

int posterior_rand(Engine* e, hipStream_t stream, const Call& c, const double* eps_t, const double* eps_e, const double* eps0_host, double* y_out, double* lml_out,
                   std::string* err) {
    auto fail = [&](hipError_t rc, const char* what) {
        if (err) *err = std::string("tgp_wide posterior draw: ") + what + ": " + hipGetErrorString(rc);
        return (int)rc;
    };
    if (!e->have || e->info.why != kOk || !e->draw_ready || e->draw_why != kOk || !c.y || !c.Rnew || !eps_t || !eps_e || !eps0_host || !y_out)
        return fail(hipErrorInvalidValue, "no plan");
    const int d = e->d, DP = e->dp, n0 = e->info.n0;
    const size_t dd = (size_t)d * d;
    const long long T = c.T;
    hipError_t rc = pinned_ready(e);
    if (rc != hipSuccess) return fail(rc, "pinned buffer");
    const size_t nf = e->tab_host.size(), nd = e->tabd_host.size();
    if (!e->draw_dev) {
        rc = tgp_alloc::dev_malloc(reinterpret_cast<void**>(&e->draw_dev), (size_t)((64 + 2) + (2 * 64 + 1)) * 64 * sizeof(double));      // (both tables at DP = 64)
        if (rc != hipSuccess) return fail(rc, "tables");
        e->draw_dev_current = false;
    }
    double *tab_f = e->draw_dev, *tab_d = tab_f + nf;
    if (!e->draw_dev_current) {
        rc = hipMemcpyAsync(tab_f, e->tab_host.data(), nf * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc == hipSuccess) rc = hipMemcpyAsync(tab_d, e->tabd_host.data(), nd * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc != hipSuccess) return fail(rc, "table upload");
        e->draw_dev_current = true;
    }
    rc = grow(e->rbuf, e->rbuf_cap, (size_t)T * sizeof(double));
    if (rc != hipSuccess) return fail(rc, "innovation buffer");
    const size_t npin = (size_t)n0 * (d + 2) + 64;
    if (npin > e->draw_pin_cap) {
        if (e->draw_pin) (void)tgp_alloc::host_free(e->draw_pin);
        e->draw_pin = nullptr;
        e->draw_pin_cap = 0;
        rc = tgp_alloc::host_malloc(reinterpret_cast<void**>(&e->draw_pin), npin * sizeof(double), hipHostMallocDefault);
        if (rc != hipSuccess) return fail(rc, "pinned buffer");
        e->draw_pin_cap = npin;
    }
    double *yh = e->pinned + pin::yh, *Rh = e->pinned + pin::Rh, *hth = e->pinned + pin::hth, *part = e->pinned + pin::part;
    double *eth = e->draw_pin, *eeh = eth + (size_t)n0 * d, *outh = eeh + n0, *dlh = outh + n0;
    rc = hipMemcpyAsync(yh, c.y, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess) rc = hipMemcpyAsync(Rh, c.Rnew, (size_t)(c.rnew_per_step ? n0 : 1) * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess && c.h_t) rc = hipMemcpyAsync(hth, c.h_t, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess) rc = hipMemcpyAsync(eth, eps_t, (size_t)n0 * d * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess) rc = hipMemcpyAsync(eeh, eps_e, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream);
    if (rc != hipSuccess) return fail(rc, "head inputs");
    ZArg z0, xT;
    const double quad = head_forward(e, yh, c.h_t ? hth : nullptr, z0, &e->head_r, nullptr);
    for (int i = 0; i < 64; ++i) {      // dl_(T-1) = chol(P_(T-1) + 1e-12 I).U' eps_0
        double s = 0.0;
        if (i < d)
            for (int k = 0; k <= i; ++k) s += e->Uend[(size_t)k * d + i] * eps0_host[k];
        xT.z[i] = s;
    }
    launch_forward(e, stream, true, tab_f, c.y, T, z0, part, e->rbuf, c.h_t, nullptr);
    rc = hipGetLastError();
    if (rc != hipSuccess) return fail(rc, "launch");
    const long long len = e->info.draw_chunk_len, halo = e->info.halo_draw;
    const unsigned chunks = (unsigned)e->info.draw_chunks;
    const double rs = e->R / e->Sss;
    if (DP == 32)
        hipLaunchKernelGGL(k_wide_post_rand<32>, dim3(chunks), dim3(64), 0, stream, tab_d, c.y, e->rbuf, eps_t, eps_e, c.Rnew, c.rnew_per_step, rs, T, (long long)n0, len, halo, d, d,
                           xT, y_out, dlh);
    else
        hipLaunchKernelGGL(k_wide_post_rand<64>, dim3(chunks), dim3(64), 0, stream, tab_d, c.y, e->rbuf, eps_t, eps_e, c.Rnew, c.rnew_per_step, rs, T, (long long)n0, len, halo, d, d,
                           xT, y_out, dlh);
    rc = hipGetLastError();
    if (rc != hipSuccess) return fail(rc, "launch");
    rc = hipStreamSynchronize(stream);
    if (rc != hipSuccess) return fail(rc, "kernel");
    // ---- the head on the host: y*_t = y_t - (R / S_t) r_t + h . dl_t + sqrt(Rnew_t) e_t; dl_(t-1) = G_t (dl_t + K_t r_t) + U_t' eps_t
    {
        const double* h = e->hvec.data();
        std::vector<double> dl(dlh, dlh + d), v(d), dn(d);
        for (int t = n0 - 1; t >= 0; --t) {
            const double r = e->head_r[t], St = e->St[t];
            const double *Kt = e->Kt.data() + (size_t)t * d, *Gt = e->Gd.data() + (size_t)t * dd, *Ut = e->Ud.data() + (size_t)t * dd, *et = eth + (size_t)t * d;
            double hx = 0.0;
            for (int i = 0; i < d; ++i) {
                hx += h[i] * dl[i];
                v[i] = dl[i] + Kt[i] * r;
            }
            outh[t] = (yh[t] - (e->R / St) * r) + hx + std::sqrt(Rh[c.rnew_per_step ? t : 0]) * eeh[t];
            for (int i = 0; i < d; ++i) {
                double s = 0.0;
                for (int k = 0; k < d; ++k) s += Gt[(size_t)i * d + k] * v[k];
                for (int k = 0; k <= i; ++k) s += Ut[(size_t)k * d + i] * et[k];
                dn[i] = s;
            }
            dl.swap(dn);
        }
    }
    rc = hipMemcpyAsync(y_out, outh, (size_t)n0 * sizeof(double), hipMemcpyHostToDevice, stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream);
    if (rc != hipSuccess) return fail(rc, "head outputs");
    *lml_out = closing_lml(e, T, quad, part);
    return 0;
}

int adjoint(Engine* e, hipStream_t stream, const ModelHost& m, long long T, const double* y, double* lml_out, const tgp_adjoint::Out& out, bool* declined,
            std::string* err) {
    *declined = true;
    auto fail = [&](hipError_t rc, const char* what) {
        if (err) *err = std::string("tgp_wide adjoint: ") + what + ": " + hipGetErrorString(rc);
        return (int)rc;
    };
    if (!e->have || e->info.why != kOk || e->d != m.d) return 0;
    const int d = e->d, n0 = e->info.n0;
    const size_t dd = (size_t)d * d;
    const double* A = e->A.data();
    // ---- the backward table: Psi = (I - h K') A' of the stationary step, gains h / S (no observer); the halo of Psi
    if (!e->adj_ready) {
        std::vector<double> AK(d), Psi(dd);
        back_step(e, e->Kt.data() + (size_t)(n0 - 1) * d, AK, Psi);
        const long long hb = halo_of(d, Psi);
        e->adj_halo = hb < 0 ? -1 : (int)hb;
        back_table(e, Psi, nullptr, e->taba_host);
        e->adj_ready = true;
        if (e->adj_dev) {      // (tables of an earlier model)
            (void)tgp_alloc::dev_free(e->adj_dev);
            e->adj_dev = nullptr;
        }
    }
    if (e->adj_halo < 0) return 0;
    const int NT = (d + 2 + 15) / 16;
    const int NG = 16 * NT, ng2 = NG * NG;
    hipError_t rc;
    // ---- buffers: tables and G (device), G and the head's end state (pinned), the per-step scratch (2 T d + T doubles), the waves' partials of G
    const size_t nf = e->tab_host.size(), nb = e->taba_host.size();
    if (!e->adj_dev) {
        rc = tgp_alloc::dev_malloc(reinterpret_cast<void**>(&e->adj_dev), (nf + nb + (size_t)ng2) * sizeof(double));
        if (rc != hipSuccess) return fail(rc, "tables");
        rc = hipMemcpyAsync(e->adj_dev, e->tab_host.data(), nf * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc == hipSuccess) rc = hipMemcpyAsync(e->adj_dev + nf, e->taba_host.data(), nb * sizeof(double), hipMemcpyHostToDevice, stream);
        if (rc != hipSuccess) return fail(rc, "table upload");
    }
    double *tab_f = e->adj_dev, *tab_b = tab_f + nf, *G_dev = tab_b + nb;
    if (!e->adj_pin) {
        rc = tgp_alloc::host_malloc(reinterpret_cast<void**>(&e->adj_pin), (size_t)(80 * 80 + 64) * sizeof(double), hipHostMallocDefault);
        if (rc != hipSuccess) return fail(rc, "pinned buffer");
    }
    rc = pinned_ready(e);
    if (rc != hipSuccess) return fail(rc, "pinned buffer");
    const size_t nTd = (size_t)T * d * sizeof(double);
    rc = grow(e->mbuf, e->mbuf_cap, nTd);
    if (rc == hipSuccess) rc = grow(e->lbuf, e->lbuf_cap, nTd);
    if (rc != hipSuccess) return fail(rc, "per-step scratch");
    rc = grow(e->rbuf, e->rbuf_cap, (size_t)T * sizeof(double));
    if (rc != hipSuccess) return fail(rc, "innovation buffer");
    // the reduction's waves: at most 2048, none with fewer than 256 steps (a multiple of four: four waves per block)
    const long long Tb = T - n0;
    long long nw = std::min<long long>(2048, std::max<long long>(1, (Tb + 255) / 256));
    nw = (nw + 3) / 4 * 4;
    long long span = (Tb + nw - 1) / nw;
    span = (span + 3) / 4 * 4;
    rc = grow(e->gpart, e->gpart_cap, (size_t)nw * ng2 * sizeof(double));
    if (rc != hipSuccess) return fail(rc, "partial sums");
    double *yh = e->pinned + pin::yh, *lam = e->pinned + pin::lam, *part = e->pinned + pin::part;
    double *Gh = e->adj_pin, *zend = Gh + 80 * 80;
    rc = hipMemcpyAsync(yh, y, (size_t)n0 * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream);
    if (rc != hipSuccess) return fail(rc, "head observations");
    // ---- the head forward: its end state m_(n0 - 1) starts chunk 0 and is the reduction's m row n0 - 1
    ZArg z0;
    const double quad = head_forward(e, yh, nullptr, z0, nullptr, nullptr);
    std::memcpy(zend, z0.z, (size_t)d * sizeof(double));
    rc = hipMemcpyAsync(e->mbuf + (size_t)(n0 - 1) * d, zend, (size_t)d * sizeof(double), hipMemcpyHostToDevice, stream);
    if (rc != hipSuccess) return fail(rc, "head's end state");
    // ---- forward (innovations and filtered means of the steps behind the head), backward (lam_t), the sums
    double *rb = e->rbuf, *mb = e->mbuf, *lb = e->lbuf;
    launch_forward(e, stream, true, tab_f, y, T, z0, part, rb, nullptr, mb);
    launch_backward(e, stream, true, tab_b, nullptr, T, y, rb, Call{}, lam, lb);
    const unsigned gblocks = (unsigned)(nw / 4);
    switch (NT) {
        case 1: hipLaunchKernelGGL(k_wide_gram<1>, dim3(gblocks), dim3(256), 0, stream, lb, mb, rb, (long long)n0, T, span, d, e->gpart); break;
        case 2: hipLaunchKernelGGL(k_wide_gram<2>, dim3(gblocks), dim3(256), 0, stream, lb, mb, rb, (long long)n0, T, span, d, e->gpart); break;
        case 3: hipLaunchKernelGGL(k_wide_gram<3>, dim3(gblocks), dim3(256), 0, stream, lb, mb, rb, (long long)n0, T, span, d, e->gpart); break;
        case 4: hipLaunchKernelGGL(k_wide_gram<4>, dim3(gblocks), dim3(256), 0, stream, lb, mb, rb, (long long)n0, T, span, d, e->gpart); break;
        default: hipLaunchKernelGGL(k_wide_gram<5>, dim3(gblocks), dim3(256), 0, stream, lb, mb, rb, (long long)n0, T, span, d, e->gpart); break;
    }
    hipLaunchKernelGGL(k_wide_gram_sum, dim3((unsigned)((ng2 + 63) / 64)), dim3(256), 0, stream, e->gpart, nw, ng2, G_dev);
    rc = hipGetLastError();
    if (rc != hipSuccess) return fail(rc, "launch");
    rc = hipMemcpyAsync(Gh, G_dev, (size_t)ng2 * sizeof(double), hipMemcpyDeviceToHost, stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream);
    if (rc != hipSuccess) return fail(rc, "kernel");
    // ---- the record of tgp_adjoint_host.hpp: SA = Glm A' + Sa a', Srm = A Grm + Sr a (mu_t = A m_(t-1) + a); psi and mu at the head's end
    const int DD = d * d, NS = DD + 3 * d + 2;
    std::vector<double> rec((size_t)3 * DD + 8 * d + 8 + d * (d + 1) / 2, 0.0);
    double *SA = rec.data(), *Sa = SA + DD, *Sk = Sa + d, *Srm = Sk + d;
    auto Gat = [&](int i, int j) { return Gh[(size_t)i * NG + j]; };
    const double Sr = Gat(d, d + 1);
    for (int i = 0; i < d; ++i) {
        Sa[i] = Gat(i, d + 1);
        Sk[i] = Gat(i, d);
        double x = Sr * e->avec[i];
        for (int j = 0; j < d; ++j) x += A[(size_t)i * d + j] * Gat(d, j);
        Srm[i] = x;
        for (int k = 0; k < d; ++k) {
            double s = Sa[i] * e->avec[k];
            for (int j = 0; j < d; ++j) s += Gat(i, j) * A[(size_t)k * d + j];
            SA[(size_t)i * d + k] = s;
        }
    }
    rec[DD + 3 * d] = Sr;
    rec[DD + 3 * d + 1] = Gat(d, d);
    for (int i = 0; i < d; ++i) {
        rec[NS + i] = lam[i];
        double x = e->avec[i];
        for (int k = 0; k < d; ++k) x += A[(size_t)i * d + k] * zend[k];
        rec[NS + d + i] = x;
    }
    double* meta = rec.data() + NS + 2 * d;
    meta[0] = (double)(n0 - 1);      // (the settled gain's index: step n0 - 1 already runs with it)
    meta[1] = 0.0;
    meta[2] = (double)T;
    meta[3] = 1.0;
    double* md = meta + 4;
    std::memcpy(md, m.A, dd * sizeof(double));
    std::memcpy(md + dd, m.a, d * sizeof(double));
    std::memcpy(md + dd + d, m.Q, dd * sizeof(double));
    std::memcpy(md + 2 * dd + d, m.H, d * sizeof(double));
    md[2 * dd + 2 * d] = m.hh;
    md[2 * dd + 2 * d + 1] = m.R;
    double* x0 = md + 2 * dd + 2 * d + 2;
    for (int i = 0; i < d; ++i) x0[i] = m.x0m[i];
    for (int c = 0; c < d; ++c)
        for (int r = 0; r <= c; ++r) x0[d + c * (c + 1) / 2 + r] = m.x0P[r + (size_t)c * d];
    const auto t_fin = std::chrono::steady_clock::now();
    tgp_wide_adjoint::Head hd;
    hd.K = e->Kt.data();
    hd.S = e->St.data();
    hd.Pf = e->Pf_head.size() == (size_t)n0 * dd ? e->Pf_head.data() : nullptr;
    hd.n = n0;
    if (tgp_wide_adjoint::finish(d, rec.data(), yh, n0, n0, out, &hd) != 0) return fail(hipErrorInvalidValue, "inconsistent record");
    e->info.finish_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_fin).count();
    *lml_out = closing_lml(e, T, quad, part);
    *declined = false;
    return 0;
}

int adjoint_finish_host(int d, const double* rec, const double* yh, long long nyh, long long head_steps, const tgp_adjoint::Out& out) {
    static const bool cpu_ok = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");      // (this object's host code is built with both)
    if (!cpu_ok) return -1;
    return tgp_wide_adjoint::finish(d, rec, yh, nyh, head_steps, out, nullptr);
}

int rand(Engine* e, hipStream_t stream, const ModelHost& m, long long T, const double* x0_host, const double* eps_t, const double* eps_e, double* y_out, bool* declined,
         std::string* err) {
    *declined = true;
    auto fail = [&](hipError_t rc, const char* what) {
        if (err) *err = std::string("tgp_wide: ") + what + ": " + hipGetErrorString(rc);
        return (int)rc;
    };
    static const bool cpu_ok = __builtin_cpu_supports("avx2") && __builtin_cpu_supports("fma");
    const int d = m.d;
    if (!cpu_ok || !supports(d) || T < 256) return 0;
    const size_t dd = (size_t)d * d;
    const int DP = d <= 31 ? 32 : 64;
    // row-major A; U = chol(Q + 1e-9 I) (upper, row-major); the open loop's halo
    std::vector<double> A(dd), U(dd, 0.0);
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < d; ++k) A[(size_t)i * d + k] = m.A[i + (size_t)k * d];
    for (int j = 0; j < d; ++j)
        for (int i = 0; i <= j; ++i) {
            double acc = 0.5 * (m.Q[i + (size_t)j * d] + m.Q[j + (size_t)i * d]) + (i == j ? 1e-9 : 0.0);
            for (int k = 0; k < i; ++k) acc -= U[(size_t)k * d + i] * U[(size_t)k * d + j];
            if (i == j) {
                if (!(acc > 0.0)) return 0;      // (not positive definite: the engines of before report it)
                U[(size_t)j * d + j] = std::sqrt(acc);
            } else {
                U[(size_t)i * d + j] = acc / U[(size_t)i * d + i];
            }
        }
    const long long halo = halo_of(d, A);
    if (halo < 0 || halo > T / 4) return 0;      // (an open loop that does not forget -- ApproxPeriodicKernel() alone: |lambda| = 1 -- or hardly)
    long long chunks = std::min<long long>(kMaxChunks, std::max<long long>(1, T / std::max<long long>(64, halo / 2)));
    const long long len = (T + chunks - 1) / chunks;
    chunks = (T + len - 1) / len;
    std::vector<double> tab((size_t)(2 * DP + 1) * 64, 0.0);
    double ha = m.hh;
    for (int i = 0; i < d; ++i) ha += m.H[i] * m.a[i];
    for (int i = 0; i < d; ++i) {
        for (int j = 0; j < d; ++j) {
            tab[(size_t)j * 64 + i] = A[(size_t)i * d + j];
            tab[(size_t)(DP + j) * 64 + i] = U[(size_t)j * d + i];      // U'[i][j]
        }
        tab[(size_t)(2 * DP) * 64 + i] = m.a[i];
    }
    for (int j = 0; j < d; ++j) {
        double gj = 0.0, uh = 0.0;
        for (int i = 0; i < d; ++i) {
            gj += m.H[i] * A[(size_t)i * d + j];
            uh += U[(size_t)j * d + i] * m.H[i];
        }
        tab[(size_t)j * 64 + d] = gj;
        tab[(size_t)(DP + j) * 64 + d] = uh;
    }
    tab[(size_t)(2 * DP) * 64 + d] = ha;
    hipError_t rc;
    const size_t need = tab.size() * sizeof(double);
    rc = grow(e->rand_dev, e->rand_cap, need);
    if (rc != hipSuccess) return fail(rc, "rand table");
    rc = hipMemcpyAsync(e->rand_dev, tab.data(), need, hipMemcpyHostToDevice, stream);
    if (rc == hipSuccess) rc = hipStreamSynchronize(stream);      // (tab is a temporary)
    if (rc != hipSuccess) return fail(rc, "rand table upload");
    ZArg x0;
    for (int i = 0; i < 64; ++i) x0.z[i] = i < d ? x0_host[i] : 0.0;
    const double sqrtR = std::sqrt(m.R);
    if (DP == 32)
        hipLaunchKernelGGL(k_wide_rand<32>, dim3((unsigned)chunks), dim3(64), 0, stream, e->rand_dev, eps_t, eps_e, sqrtR, T, len, halo, d, d, x0, y_out);
    else
        hipLaunchKernelGGL(k_wide_rand<64>, dim3((unsigned)chunks), dim3(64), 0, stream, e->rand_dev, eps_t, eps_e, sqrtR, T, len, halo, d, d, x0, y_out);
    rc = hipGetLastError();
    if (rc != hipSuccess) return fail(rc, "launch");
    *declined = false;
    return 0;
}

}  // namespace tgp_wide
