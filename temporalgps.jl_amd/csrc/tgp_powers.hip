// The dense-power one-launch kernels -- k_rand_one, k_filter_one, k_adjoint_one, k_smooth_one -- with their launch code and host plans: see
// tgp_powers.hpp.  gfx950 only (wave64, DPP scans, uniform coefficients through the kernel-argument segment).
//
// All four walk one skeleton: a workgroup owns a span of the series and starts its 8 tiles a halo earlier; a lane runs its 8 steps from a zero
// state, the lanes' end states are scanned inside the tile, the tiles are chained over the <= 3 tiles before them, and the lane's true start
// state gives its outputs; the adjoint and the smoother do the same backwards.  The steps of that skeleton every kernel takes alike are the
// building blocks below, written once; what a kernel computes with them -- its sweeps, outputs, sums and hand-overs -- stands in its own body.
#include "tgp_powers.hpp"
#include "tgp_lane.hpp"
#include "tgp_modal.hpp"

#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace tgp_powers {

namespace {

constexpr int kWJ = tgp_plan::kSub;      // steps per lane; rows of the WJ / WG tables
constexpr int kNW = 8;                   // waves per workgroup: 8 tiles of 512 steps

// ---- the shared blocks.  The kernels read their arguments in place from the kernel-argument segment, so that coefficients arrive by scalar
// loads: a block takes the argument tables by reference, is always inlined, and indexes them with compile-time constants only (a run-time
// index, or a call that is not inlined, would make the compiler keep a copy of the arguments in scratch memory).

// The span of this workgroup: consecutive workgroups (they share their halos' lines) on the same XCD.  false: the block has none.
__device__ __forceinline__ bool span_of_block(long long nwg, long long* g) {
    const long long per = (nwg + 7) / 8;
    *g = (long long)(blockIdx.x & 7) * per + (blockIdx.x >> 3);
    return (long long)(blockIdx.x >> 3) < per && *g < nwg;
}

// y += M x, or M' x (dense, M from the kernel arguments)
template <int D, bool TRANSPOSED = false>
__device__ __forceinline__ void matvec_acc(const double (&M)[D][D], const double (&x)[D], double (&y)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double v = y[i];
#pragma unroll
        for (int k = 0; k < D; ++k) v = fma(TRANSPOSED ? M[k][i] : M[i][k], x[k], v);
        y[i] = v;
    }
}
// y += M^(8 e) x, or its transpose, from a per-lane power table
template <int D, bool TRANSPOSED = false>
__device__ __forceinline__ void table_acc(const double (&sPw)[D][D][64], int e, const double (&x)[D], double (&y)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
        for (int k = 0; k < D; ++k) y[i] = fma(TRANSPOSED ? sPw[k][i][e] : sPw[i][k][e], x[k], y[i]);
}

// Row i of M^(8 lane) by the bits of the lane number (P[b] = M^(8 2^b))
template <int D>
__device__ __forceinline__ void power_row(const double (&P)[6][D][D], int i, int lane, double (&row)[D]) {
#pragma unroll
    for (int k = 0; k < D; ++k) row[k] = (k == i) ? 1.0 : 0.0;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        double nr[D];
#pragma unroll
        for (int k = 0; k < D; ++k) {
            double v = 0.0;
#pragma unroll
            for (int m = 0; m < D; ++m) v = fma(row[m], P[b][m][k], v);
            nr[k] = v;
        }
        const bool bit = ((lane >> b) & 1) != 0;
#pragma unroll
        for (int k = 0; k < D; ++k) row[k] = bit ? nr[k] : row[k];
    }
}
// The per-lane power table sPw[i][k][lane] of M, its rows shared out over the waves (wave-uniform).  A barrier stands between this and the first read.
template <int D, int NW>
__device__ __forceinline__ void build_power_table(const double (&P)[6][D][D], double (&sPw)[D][D][64], int lane, int wave) {
    const int uw = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        if (uw != i % NW) continue;
        double row[D];
        power_row<D>(P, i, lane, row);
#pragma unroll
        for (int k = 0; k < D; ++k) sPw[i][k][lane] = row[k];
    }
}

// A lane's SUB observations minus the emission offset: 16-byte loads where the series and the pointer allow, zero behind the series' end
template <int SUB>
__device__ __forceinline__ void load_lane_obs(const double* y, long long t0, long long T, double hh, double (&u)[SUB]) {
    if (t0 + SUB <= T && (reinterpret_cast<uintptr_t>(y) & 15) == 0) {
        const v2d* q = reinterpret_cast<const v2d*>(y + t0);
#pragma unroll
        for (int j = 0; j < SUB / 2; ++j) {
            const v2d w = q[j];
            u[2 * j] = w.x - hh;
            u[2 * j + 1] = w.y - hh;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SUB; ++j) u[j] = t0 + j < T ? y[t0 + j] - hh : 0.0;
    }
}

// One level of the in-row scans: x += P[K] (x shifted by 2^K lanes inside the row of 16), from below -- or, BACK, from above
template <int D, int K, bool BACK, bool TRANSPOSED>
__device__ __forceinline__ void scan_level(const double (&P)[6][D][D], double (&x)[D]) {
    double g[D], n[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        g[i] = dpp_mov<(BACK ? 0x100 : 0x110) + (1 << K)>(x[i]);
        n[i] = x[i];
    }
    matvec_acc<D, TRANSPOSED>(P[K], g, n);
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = n[i];
}

// Inclusive scan of the lanes' end states over the tile: x_l <- sum_{m <= l} M^(8 (l - m)) x_m.  Rows of 16 by DPP moves on P, then across
// the rows (row_bcast:15, :31) through the per-lane table.
template <int D>
__device__ __forceinline__ void scan_forward(const double (&P)[6][D][D], const double (&sPw)[D][D][64], int lane, double (&x)[D]) {
    scan_level<D, 0, false, false>(P, x);
    scan_level<D, 1, false, false>(P, x);
    scan_level<D, 2, false, false>(P, x);
    scan_level<D, 3, false, false>(P, x);
    const int e1 = (lane & 15) + 1, e2 = lane >= 32 ? lane - 31 : 0;
    double gv[D], nv[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        gv[i] = dpp_mov<0x142, 0xA>(x[i]);
        nv[i] = x[i];
    }
    table_acc<D>(sPw, e1, gv, nv);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        x[i] = nv[i];
        gv[i] = dpp_mov<0x143, 0xC>(nv[i]);
    }
    table_acc<D>(sPw, e2, gv, nv);
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = nv[i];
}
// The scanned tile hands on: st, the state in front of the lane's steps (its left neighbour's; lane 0: zero), and the tile's end state to sF
// (zero from a tile with nothing to do).  A barrier stands between this and chain_forward.
template <int D>
__device__ __forceinline__ void end_forward(const double (&x)[D], bool any_valid, int lane, double (&sFw)[D], double (&st)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) st[i] = dpp_mov<0x138>(x[i]);
    if (lane == 63) {
#pragma unroll
        for (int i = 0; i < D; ++i) sFw[i] = any_valid ? x[i] : 0.0;
    }
}
// The tile's start state from the <= 3 tiles before it (PT = M^512, M^1024), into the lanes' start states.  from_x0: the state x0 sits at
// position -1 of the workgroup's tiles (wave-uniform) -- the drawn state, or the head's end state.
template <int D, int NW>
__device__ __forceinline__ void chain_forward(const double (&PT)[2][D][D], const double (&sF)[NW][D], const double (&sPw)[D][D][64], int wave, int lane,
                                              bool from_x0, const double (&x0)[D], double (&st)[D]) {
    double zin[D];
#pragma unroll
    for (int i = 0; i < D; ++i) zin[i] = 0.0;
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
        const int src = wave - k;
        if (src < -1 || (src == -1 && !from_x0)) continue;      // (wave-uniform)
        double xs[D];
#pragma unroll
        for (int i = 0; i < D; ++i) xs[i] = src >= 0 ? sF[src][i] : x0[i];
        if (k == 1) {
#pragma unroll
            for (int i = 0; i < D; ++i) zin[i] += xs[i];
        } else {
            matvec_acc<D>(PT[k - 2], xs, zin);
        }
    }
    table_acc<D>(sPw, lane, zin, st);
}

// Reverse scan over the tile: x_l <- sum_{m >= l} N^(8 (m - l)) x_m with N = M, or, TRANSPOSED, N = M' (the same tables read the other way).
// Rows by row_shl moves; rows 0 and 2 then take the first lane of the row above them, the lower half takes lane 32.
template <int D, bool TRANSPOSED>
__device__ __forceinline__ void scan_backward(const double (&P)[6][D][D], const double (&sPw)[D][D][64], int lane, double (&x)[D]) {
    scan_level<D, 0, true, TRANSPOSED>(P, x);
    scan_level<D, 1, true, TRANSPOSED>(P, x);
    scan_level<D, 2, true, TRANSPOSED>(P, x);
    scan_level<D, 3, true, TRANSPOSED>(P, x);
    const int e1 = 16 - (lane & 15);      // 16 - p lanes away
    double gv[D], nv[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        gv[i] = dpp_mov<0x15F, 0x5>(dpp_mov<0x130>(x[i]));
        nv[i] = x[i];
    }
    table_acc<D, TRANSPOSED>(sPw, e1, gv, nv);
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = nv[i];
    const int e2 = lane < 32 ? 32 - lane : 0;
    const double keep = lane < 32 ? 1.0 : 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) gv[i] = readlane_d(x[i], 32) * keep;
    table_acc<D, TRANSPOSED>(sPw, e2, gv, nv);
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = nv[i];
}
// end_forward's mirror: pin, the state behind the lane's last step (its right neighbour's; lane 63: zero), and the tile's first state to sB
template <int D>
__device__ __forceinline__ void end_backward(const double (&x)[D], bool any_valid, int lane, double (&sBw)[D], double (&pin)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) pin[i] = dpp_mov<0x130>(x[i]);
    if (lane == 0) {
#pragma unroll
        for (int i = 0; i < D; ++i) sBw[i] = any_valid ? x[i] : 0.0;
    }
}
// chain_forward's mirror over the <= 3 tiles behind; zin: what enters the tile from behind (k_smooth_one hands it on to the host)
template <int D, int NW, bool TRANSPOSED>
__device__ __forceinline__ void chain_backward(const double (&PT)[2][D][D], const double (&sB)[NW][D], const double (&sPw)[D][D][64], int wave, int lane,
                                               double (&zin)[D], double (&pin)[D]) {
#pragma unroll
    for (int i = 0; i < D; ++i) zin[i] = 0.0;
#pragma unroll
    for (int k = 1; k <= 3; ++k) {
        const int src = wave + k;
        if (src >= NW) continue;
        if (k == 1) {
#pragma unroll
            for (int i = 0; i < D; ++i) zin[i] += sB[src][i];
        } else {
            matvec_acc<D, TRANSPOSED>(PT[k - 2], sB[src], zin);
        }
    }
    table_acc<D, TRANSPOSED>(sPw, 63 - lane, zin, pin);
}

// One wave hands the head's nhs observations to the host through pinned memory and raises the flag (2 seq) behind everything it has written
// there -- whatever else the head needs goes in before the call.
__device__ __forceinline__ void send_head_in(double* head_in, long long* flag, long long seq, const double* y, long long nhs, int lane) {
    for (long long t = lane; t < nhs; t += 64) head_in[t] = y[t];
    __threadfence_system();
    if (lane == 0) __hip_atomic_store(flag, 2 * seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ---- host side
template <int D>
void fill_powers(double (&P)[6][D][D], double (&PT)[2][D][D], const double (&src_P)[6][tgp_plan::kRandMaxD * tgp_plan::kRandMaxD],
                 const double (&src_PT)[2][tgp_plan::kRandMaxD * tgp_plan::kRandMaxD]) {
    for (int i = 0; i < D; ++i)
        for (int k = 0; k < D; ++k) {
            for (int b = 0; b < 6; ++b) P[b][i][k] = src_P[b][i * D + k];
            for (int b = 0; b < 2; ++b) PT[b][i][k] = src_PT[b][i * D + k];
        }
}
// one block per span, dealt over the 8 XCDs (span_of_block)
template <class KA>
int launch_spans(void (*kernel)(const KA), long long nwg, hipStream_t st, const KA& ka) {
    const long long per = (nwg + 7) / 8;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(per * 8)), dim3(kNW * 64), 0, st, ka);
    return (int)hipGetLastError();
}
// The state dimension as a compile-time constant: f(dim<d>{}) for 1 <= d <= MAXD (6 or 8)
template <int N>
using dim = std::integral_constant<int, N>;
template <int MAXD, class F>
int dispatch_d(int d, F&& f) {
    static_assert(MAXD == 6 || MAXD == 8, "the d limits of the kernels");
    switch (d) {
        case 1: return f(dim<1>{});
        case 2: return f(dim<2>{});
        case 3: return f(dim<3>{});
        case 4: return f(dim<4>{});
        case 5: return f(dim<5>{});
        case 6: return f(dim<6>{});
        case 7: if constexpr (MAXD >= 7) return f(dim<7>{}); else break;
        case 8: if constexpr (MAXD >= 8) return f(dim<8>{}); else break;
    }
    return (int)hipErrorInvalidValue;
}

// =================================================================================================================================
// rand of an LTI model (lgssm.jl:65-91, the draws supplied): x_t = A x_{t-1} + a + Lq eps_t,  y_t = h' x_t + hh + sqrt(R) eta_t.
// The same one-launch structure as k_steady_one, forwards only and on DENSE powers (the open-loop transition of a Matern-3/2 / -5/2 block is
// a Jordan block: no modal form).  Workgroup g owns the outputs [g C, (g + 1) C), C = 8 tiles of 512 steps minus the halo; its tiles start
// `halo` steps earlier from a zero state (g = 0: at step 0 from the drawn x0); a lane runs its 8 steps from zero, the lanes' end states are
// scanned (rows of 16 by DPP moves with A^(8 2^k), across the rows through a per-lane table of A^(8 e) in LDS), the tiles are chained over
// the <= 3 tiles before them, and the lane's start state reaches its 8 outputs through the rows h' A^(j+1).  Reads eps_t (8 d B/step) and
// eps_e once, writes y once.
// =================================================================================================================================
template <int D>
struct RArgs {
    double A[D][D], a[D], Lq[D][D], h[D], hh, sR;
    double P[6][D][D];       // A^(8 2^k)
    double PT[2][D][D];      // A^512, A^1024
    double WJ[kWJ][D];       // h' A^(j+1)
    double x0[D];
    long long T, C, nwg;
    int halo;
    const double *eps_t, *eps_e;
    double* y;
};

template <int D, int NW>
__global__ __launch_bounds__(NW * 64, (D <= 4 ? 4 : 2)) void k_rand_one(const RArgs<D> by_value) {
    (void)by_value;
    const RArgs<D>& ka = *(const RArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();      // (read in place: see k_steady_one)
    constexpr int SUB = kWJ, TILE = 64 * SUB;
    __shared__ double sF[NW][D];
    __shared__ double sPw[D][D][64];      // A^(8 e), e = 0 .. 63: entry [i][k][e]
    constexpr int LV = SUB * D / 2;       // 16-byte pieces of draws per lane
    __shared__ v2d sT[NW][16 * (LV + 1)];      // a quarter of a tile's draws on their way from memory order to the lanes (one spare piece per lane:
                                               // the 16 reading lanes then start in 16 different groups of four banks)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long g;
    if (!span_of_block(ka.nwg, &g)) return;
    const long long T = ka.T, c_lo = g * ka.C, c_hi = (c_lo + ka.C < T) ? c_lo + ka.C : T;
    const bool first = g == 0;
    const long long s0 = first ? 0 : c_lo - ka.halo;
    const long long tile_t0 = s0 + (long long)wave * TILE, t0 = tile_t0 + (long long)lane * SUB;
    const bool any_valid = tile_t0 < c_hi;      // (wave-uniform: a tile wholly behind the workgroup's range has nothing to do)
    build_power_table<D, NW>(ka.P, sPw, lane, wave);
    // ---- the lane's eight steps from a zero state
    double y0[SUB], x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) y0[j] = 0.0;
    if (any_valid) {
        const bool whole = t0 + SUB <= T && (reinterpret_cast<uintptr_t>(ka.eps_t) & 15) == 0 && (reinterpret_cast<uintptr_t>(ka.eps_e) & 15) == 0;
        // a whole tile's draws are 64 SUB D consecutive doubles: fetched in memory order (every load instruction 1 KB of consecutive bytes;
        // a lane fetching its own SUB D values, 16 bytes at a stride of 8 SUB D, keeps the address path busy four to eight times as long)
        // and handed to their lanes through LDS, sixteen lanes' worth at a time
        const bool tile_whole = tile_t0 + TILE <= T && (reinterpret_cast<uintptr_t>(ka.eps_t) & 15) == 0 && ((tile_t0 * D) & 1) == 0;      // (wave-uniform)
        double evt[SUB * D];
        if (tile_whole) {
            const v2d* src = reinterpret_cast<const v2d*>(ka.eps_t + tile_t0 * D);
            v2d ld[4][D];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int i = 0; i < D; ++i) ld[r][i] = src[r * 16 * LV + i * 64 + lane];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    const int idx = i * 64 + lane;
                    sT[wave][idx + idx / LV] = ld[r][i];
                }
                lds_sync();
                if ((lane >> 4) == r) {
#pragma unroll
                    for (int k = 0; k < LV; ++k) {
                        const v2d w = sT[wave][(lane & 15) * (LV + 1) + k];
                        evt[2 * k] = w.x;
                        evt[2 * k + 1] = w.y;
                    }
                }
                lds_sync();
            }
        }
        double ee[SUB];
        if (whole) {
            const v2d* q = reinterpret_cast<const v2d*>(ka.eps_e + t0);
#pragma unroll
            for (int j = 0; j < SUB / 2; ++j) {
                const v2d w = q[j];
                ee[2 * j] = w.x;
                ee[2 * j + 1] = w.y;
            }
        } else {
#pragma unroll
            for (int j = 0; j < SUB; ++j) ee[j] = t0 + j < T ? ka.eps_e[t0 + j] : 0.0;
        }
#pragma unroll
        for (int j2 = 0; j2 < SUB; j2 += 2) {
            // the draws of two steps: 2 d consecutive doubles (16-byte pieces where the series allows)
            double ev[2 * D];
            if (tile_whole) {
#pragma unroll
                for (int k = 0; k < 2 * D; ++k) ev[k] = evt[j2 * D + k];
            } else if (whole) {
                const v2d* q = reinterpret_cast<const v2d*>(ka.eps_t + (t0 + j2) * D);
#pragma unroll
                for (int k = 0; k < D; ++k) {
                    const v2d w = q[k];
                    ev[2 * k] = w.x;
                    ev[2 * k + 1] = w.y;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 2 * D; ++k) ev[k] = (t0 + j2) * D + k < T * D ? ka.eps_t[(t0 + j2) * D + k] : 0.0;
            }
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = j2 + jj;
                double nx[D];
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    double v = ka.a[i];
#pragma unroll
                    for (int k = 0; k <= i; ++k) v = fma(ka.Lq[i][k], ev[jj * D + k], v);      // (lower factor)
                    nx[i] = v;
                }
                matvec_acc<D>(ka.A, x, nx);
                double yy = fma(ka.sR, ee[j], ka.hh);
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    x[i] = nx[i];
                    yy = fma(ka.h[i], nx[i], yy);
                }
                y0[j] = yy;
            }
        }
    }
    __syncthreads();      // (the table)
    // ---- inclusive scan of the lanes' end states: x_l <- sum_{m <= l} A^(8 (l - m)) x_m
    double st[D];
    if (any_valid) scan_forward<D>(ka.P, sPw, lane, x);
    end_forward<D>(x, any_valid, lane, sF[wave], st);
    __syncthreads();
    if (!any_valid) return;
    // ---- the tile's start state from the <= 3 tiles before it (workgroup 0: the drawn x0 sits at position -1), then the outputs
    chain_forward<D, NW>(ka.PT, sF, sPw, wave, lane, first, ka.x0, st);
    const bool aligned = (reinterpret_cast<uintptr_t>(ka.y) & 15) == 0;
#pragma unroll
    for (int j = 0; j < SUB; j += 2) {
        double m0 = y0[j], m1 = y0[j + 1];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            m0 = fma(ka.WJ[j][i], st[i], m0);
            m1 = fma(ka.WJ[j + 1][i], st[i], m1);
        }
        const long long t = t0 + j;
        if (t >= c_lo && t + 1 < c_hi && aligned) {
            v2d w;
            w.x = m0;
            w.y = m1;
            *reinterpret_cast<v2d*>(ka.y + t) = w;
        } else {
            if (t >= c_lo && t < c_hi) ka.y[t] = m0;
            if (t + 1 >= c_lo && t + 1 < c_hi) ka.y[t + 1] = m1;
        }
    }
}

template <int D>
int launch_rand(hipStream_t st, const tgp_plan::RandPlan& rp, const double* x0, const double* eps_t, const double* eps_e, long long T, double* y) {
    RArgs<D> ka;
    static_assert(sizeof(RArgs<D>) <= 8192, "the kernel-argument segment (12 KB launch on gfx950: scripts/micro/bigarg.hip)");
    std::memset(&ka, 0, sizeof ka);
    for (int i = 0; i < D; ++i) {
        ka.a[i] = rp.a[i];
        ka.h[i] = rp.h[i];
        ka.x0[i] = x0[i];
        for (int k = 0; k < D; ++k) {
            ka.A[i][k] = rp.A[i * D + k];
            ka.Lq[i][k] = rp.Lq[i * D + k];
        }
    }
    fill_powers<D>(ka.P, ka.PT, rp.P, rp.PT);
    for (int j = 0; j < kWJ; ++j)
        for (int i = 0; i < D; ++i) ka.WJ[j][i] = rp.WJ[j][i];
    ka.hh = rp.hh;
    ka.sR = rp.sR;
    ka.T = T;
    ka.halo = rp.halo;
    ka.C = rand_span(rp);
    ka.nwg = rand_workgroups(rp, T);
    ka.eps_t = eps_t;
    ka.eps_e = eps_e;
    ka.y = y;
    return launch_spans(k_rand_one<D, kNW>, ka.nwg, st, ka);
}
}  // namespace

int rand_lti(hipStream_t stream, const tgp_plan::RandPlan& plan, const double* x0, const double* eps_t, const double* eps_e, long long T, double* y,
             const char** kname) {
    if (kname) *kname = "k_rand_one";
    return dispatch_d<8>(plan.d, [&](auto d) { return launch_rand<decltype(d)::value>(stream, plan, x0, eps_t, eps_e, T, y); });
}

long long rand_span(const tgp_plan::RandPlan& rp) { return (long long)kNW * 64 * kWJ - rp.halo; }
long long rand_workgroups(const tgp_plan::RandPlan& rp, long long T) {
    const long long C = rand_span(rp);
    return (T + C - 1) / C;
}

// =================================================================================================================================
// _filter of an LTI model behind its head (lgssm.jl:171-187): mu' = Phi mu + a + (A K) u, r = u - h' mu, m_t = mu_t + K r_t, P_t = P_ss.
// k_rand_one's structure on the dense powers of the closed loop Phi = A - (A K) h': a first sweep of a lane's 8 steps from a zero state gives
// its end state, the scan and the tile chaining its true start state, a second sweep from there the outputs.  Workgroup 0 starts at nhs from
// the head's end state (computed on the host).  Reads y once, writes 8 (d + d^2) bytes per step.
// =================================================================================================================================
namespace {
template <int D>
struct FArgs {
    double Phi[D][D], a[D], kA[D], K[D], h[D], hh;
    double P[6][D][D], PT[2][D][D];
    double Pss[D * D];
    double Gss[D * D], Lss[D * D];      // posterior(model, y): the settled reverse-time transition and its noise, COLUMN-major as they leave
    double mu0[D];
    long long T, C, nwg, nhs;
    int halo;
    const double* y;
    double *m, *Pc, *part;
    double *Gc, *gc, *Lc, *fin;      // (all four or none) G, L [T][D D], g [T][D]; fin [D]: the last filtered mean
};

template <int D, int NW>
__global__ __launch_bounds__(NW * 64, (D <= 3 ? 4 : 2)) void k_filter_one(const FArgs<D> by_value) {      // (d = 4 at four waves per SIMD: 18 registers spilled)
    (void)by_value;
    const FArgs<D>& ka = *(const FArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int SUB = kWJ, TILE = 64 * SUB;
    __shared__ double sF[NW][D], sAcc[NW];
    __shared__ double sPw[D][D][64];      // Phi^(8 e), e = 0 .. 63
    __shared__ double sP[3][D * D];       // the settled covariance, G, L (the fills below index them per lane)
    constexpr int LV = SUB * D / 2;        // 16-byte pieces of means per lane
    __shared__ v2d sT[NW][16 * (LV + 1)];      // a quarter of a tile's means (or g) on their way from the lanes to memory order
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    long long g;
    if (!span_of_block(ka.nwg, &g)) return;
    if (threadIdx.x < D * D) {
        sP[0][threadIdx.x] = ka.Pss[threadIdx.x];
        sP[1][threadIdx.x] = ka.Gss[threadIdx.x];
        sP[2][threadIdx.x] = ka.Lss[threadIdx.x];
    }
    const long long T = ka.T, c_lo = ka.nhs + g * ka.C, c_hi = (c_lo + ka.C < T) ? c_lo + ka.C : T;
    const bool first = g == 0;
    const long long s0 = first ? ka.nhs : c_lo - ka.halo;
    const long long tile_t0 = s0 + (long long)wave * TILE, t0 = tile_t0 + (long long)lane * SUB;
    const bool any_valid = tile_t0 < c_hi;
    build_power_table<D, NW>(ka.P, sPw, lane, wave);
    // ---- first sweep: the lane's 8 steps from a zero state
    double u[SUB], x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) u[j] = 0.0;
    if (any_valid) {
        load_lane_obs<SUB>(ka.y, t0, T, ka.hh, u);
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            double nx[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double v = fma(ka.kA[i], u[j], ka.a[i]);
#pragma unroll
                for (int k = 0; k < D; ++k) v = fma(ka.Phi[i][k], x[k], v);
                nx[i] = v;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) x[i] = nx[i];
        }
    }
    __syncthreads();
    double st[D];
    if (any_valid) scan_forward<D>(ka.P, sPw, lane, x);
    end_forward<D>(x, any_valid, lane, sF[wave], st);
    __syncthreads();
    double acc = 0.0;
    if (any_valid) {
        chain_forward<D, NW>(ka.PT, sF, sPw, wave, lane, first, ka.mu0, st);
        // ---- second sweep from the true start state: innovations, filtered means
        const bool whole = t0 >= c_lo && t0 + SUB <= c_hi;
        const bool m_al = ka.m != nullptr && (reinterpret_cast<uintptr_t>(ka.m) & 15) == 0;
        // a tile wholly inside the workgroup's range (and short of the series' last step): its 512 D means -- or the 512 D values of g, one step
        // to the right -- are one run of consecutive doubles; they leave in memory order through LDS (below) instead of lane by lane
        const bool run_whole = tile_t0 >= c_lo && tile_t0 + TILE <= c_hi && tile_t0 + TILE < T;      // (wave-uniform)
        double* const run = !run_whole ? nullptr : (ka.gc != nullptr ? ka.gc + (tile_t0 + 1) * D : (ka.m != nullptr ? ka.m + tile_t0 * D : nullptr));
        const bool want_g = ka.gc != nullptr;
        double oall[SUB * D];
#pragma unroll
        for (int j2 = 0; j2 < SUB; j2 += 2) {
            double mf[2 * D];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                const int j = j2 + jj;
                double r = u[j];
#pragma unroll
                for (int k = 0; k < D; ++k) r = fma(-ka.h[k], st[k], r);
                const long long t = t0 + j;
                if (t >= c_lo && t < c_hi) acc = fma(r, r, acc);
                double nx[D];
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    mf[jj * D + i] = fma(ka.K[i], r, st[i]);
                    double v = fma(ka.kA[i], u[j], ka.a[i]);
#pragma unroll
                    for (int k = 0; k < D; ++k) v = fma(ka.Phi[i][k], st[k], v);
                    nx[i] = v;
                }
#pragma unroll
                for (int i = 0; i < D; ++i) st[i] = nx[i];
                if (run != nullptr) {
#pragma unroll
                    for (int i = 0; i < D; ++i) {
                        double v = mf[jj * D + i];
                        if (want_g) {
#pragma unroll
                            for (int k = 0; k < D; ++k) v = fma(-ka.Gss[k * D + i], nx[k], v);
                        }
                        oall[j * D + i] = v;
                    }
                } else if (ka.gc != nullptr && t >= c_lo && t < c_hi) {
                    // step t + 1 of the reverse-time model (lgssm.jl:215-221, :231-238): g = m_t - G mu_(t+1)
                    if (t + 1 < T) {
#pragma unroll
                        for (int i = 0; i < D; ++i) {
                            double v = mf[jj * D + i];
#pragma unroll
                            for (int k = 0; k < D; ++k) v = fma(-ka.Gss[k * D + i], nx[k], v);
                            ka.gc[(t + 1) * D + i] = v;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < D; ++i) ka.fin[i] = mf[jj * D + i];
                    }
                }
            }
            if (ka.m != nullptr && run == nullptr) {
                const long long t = t0 + j2;
                if (whole && m_al) {      // (t D is even: 16-byte pieces)
                    v2d* q = reinterpret_cast<v2d*>(ka.m + t * D);
#pragma unroll
                    for (int k = 0; k < D; ++k) {
                        v2d w;
                        w.x = mf[2 * k];
                        w.y = mf[2 * k + 1];
                        q[k] = w;
                    }
                } else {
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj)
                        if (t + jj >= c_lo && t + jj < c_hi)
#pragma unroll
                            for (int i = 0; i < D; ++i) ka.m[(t + jj) * D + i] = mf[jj * D + i];
                }
            }
        }
        if (run != nullptr) {
            // sixteen lanes' values at a time: in at 16-byte pieces per lane (one spare piece per lane: no bank conflicts), out as doubles in
            // memory order -- every store instruction 512 consecutive bytes (g sits D doubles off the tile's start: 8-byte granularity)
            const double* sTd = reinterpret_cast<const double*>(&sT[wave][0]);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if ((lane >> 4) == r) {
#pragma unroll
                    for (int k = 0; k < LV; ++k) {
                        v2d w;
                        w.x = oall[2 * k];
                        w.y = oall[2 * k + 1];
                        sT[wave][(lane & 15) * (LV + 1) + k] = w;
                    }
                }
                lds_sync();
#pragma unroll
                for (int i = 0; i < 2 * D; ++i) {
                    const int e = i * 64 + lane;      // of the 16 lanes' 128 D doubles
                    run[r * 128 * D + e] = sTd[e + 2 * (e / (SUB * D))];
                }
                lds_sync();
            }
        }
        // the covariances: the settled one, for every step the workgroup owns -- a whole tile as one run of 512 D^2 doubles, every store
        // instruction 1 KB of consecutive bytes (a lane writing its own 8 D^2 values, 16 bytes at a 64 D^2-byte stride: 40 % slower)
        constexpr int DD = D * D;
        const bool tile_whole = tile_t0 >= c_lo && tile_t0 + TILE <= c_hi;      // (wave-uniform)
#pragma unroll
        for (int which = 0; which < 3; ++which) {
            double* dst = which == 0 ? ka.Pc : (which == 1 ? ka.Gc : ka.Lc);
            if (dst == nullptr) continue;
            if (tile_whole && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
                v2d* q = reinterpret_cast<v2d*>(dst + tile_t0 * DD);
#pragma unroll 4
                for (int k = 0; k < SUB * DD / 2; ++k) {
                    const int e = k * 64 + lane;
                    v2d w;
                    w.x = sP[which][(2 * e) % DD];
                    w.y = sP[which][(2 * e + 1) % DD];
                    q[e] = w;
                }
            } else {
#pragma unroll
                for (int j = 0; j < SUB; ++j)
                    if (t0 + j >= c_lo && t0 + j < c_hi)
#pragma unroll
                        for (int e = 0; e < DD; ++e) dst[(t0 + j) * DD + e] = sP[which][e];
            }
        }
    }
    acc = wave_sum_to_lane63(acc);
    if (lane == 63) sAcc[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tsum = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) tsum += sAcc[w];
        ka.part[g] = tsum;
    }
}

template <int D>
int launch_filter(hipStream_t st, const tgp_plan::FilterPlan& fp, const double* mu0, const double* y, long long T, double* m, double* Pc, double* part,
                  const PosteriorOut* po) {
    FArgs<D> ka;
    static_assert(sizeof(FArgs<D>) <= 8192, "the kernel-argument segment (12 KB launch on gfx950: scripts/micro/bigarg.hip)");
    std::memset(&ka, 0, sizeof ka);
    for (int i = 0; i < D; ++i) {
        ka.a[i] = fp.a[i];
        ka.kA[i] = fp.kA[i];
        ka.K[i] = fp.K[i];
        ka.h[i] = fp.h[i];
        ka.mu0[i] = mu0[i];
        for (int k = 0; k < D; ++k) {
            ka.Phi[i][k] = fp.Phi[i * D + k];
            ka.Pss[i * D + k] = fp.Pss[i * D + k];
            if (po) {
                ka.Gss[i * D + k] = po->Gss[i * D + k];
                ka.Lss[i * D + k] = po->Lss[i * D + k];
            }
        }
    }
    fill_powers<D>(ka.P, ka.PT, fp.P, fp.PT);
    ka.hh = fp.hh;
    ka.T = T;
    ka.nhs = fp.nhs;
    ka.halo = fp.halo;
    ka.C = filter_span(fp);
    ka.nwg = filter_workgroups(fp, T);
    ka.y = y;
    ka.m = m;
    ka.Pc = Pc;
    ka.part = part;
    if (po) {
        ka.Gc = po->G;
        ka.gc = po->g;
        ka.Lc = po->L;
        ka.fin = po->fin;
    }
    return launch_spans(k_filter_one<D, kNW>, ka.nwg, st, ka);
}
}  // namespace

long long filter_span(const tgp_plan::FilterPlan& fp) { return (long long)kNW * 64 * kWJ - fp.halo; }
long long filter_workgroups(const tgp_plan::FilterPlan& fp, long long T) {
    const long long C = filter_span(fp);
    return (T - fp.nhs + C - 1) / C;
}

int filter_lti(hipStream_t stream, const tgp_plan::FilterPlan& fp, const double* mu_start, const double* y, long long T, double* m_out, double* P_out,
               double* part, const PosteriorOut* po) {
    return dispatch_d<8>(fp.d, [&](auto d) { return launch_filter<decltype(d)::value>(stream, fp, mu_start, y, T, m_out, P_out, part, po); });
}

// =================================================================================================================================
// The adjoint (gradient) pass of an LTI model behind its head, in one launch.  k_filter_one's forward half gives a lane
// its true start state; a second forward sweep keeps mu_j and r_j of its 8 steps; the adjoint psi = Phi' psi + h r / S runs the same way
// backwards (zero-start sweep, reverse scan by DPP moves on the TRANSPOSED powers -- the same table read the other way --, chaining over the
// <= 3 tiles behind); the last sweep walks the 8 steps backwards with the true psi and accumulates the d^2 + 3 d + 2 sums.  Spans carry a
// halo at both ends.
// =================================================================================================================================
namespace {
template <int D>
struct GArgs {
    double Phi[D][D], a[D], kA[D], h[D], hh, iS;
    double P[6][D][D], PT[2][D][D];
    double mu0[D];
    long long T, C, nwg, nhs;
    int halo;
    const double* y;
    double *part, *psi_out;
    // the head beside the kernel (SmoothCall in tgp_powers.hpp): workgroup 0 hands the head's observations over through pinned memory and waits
    // (bounded) for the predicted mean of step nhs; nullptr: mu0 above by value
    double* head_in;
    long long* head_in_flag;
    const double* mu0p;
    const long long* mu0_flag;
    long long seq;
};

template <int D, int NW>
__global__ __launch_bounds__(NW * 64, 2) void k_adjoint_one(const GArgs<D> by_value) {
    (void)by_value;
    const GArgs<D>& ka = *(const GArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int SUB = kWJ, TILE = 64 * SUB, NS = D * D + 3 * D + 2;
    __shared__ double sF[NW][D], sB[NW][D], sAcc[NW][NS];
    __shared__ double sPw[D][D][64];      // Phi^(8 e), e = 0 .. 63
    __shared__ double sPoison;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) sPoison = 0.0;
    long long g;
    if (!span_of_block(ka.nwg, &g)) return;
    const long long T = ka.T, c_lo = ka.nhs + g * ka.C, c_hi = (c_lo + ka.C < T) ? c_lo + ka.C : T;
    const bool first = g == 0;
    const bool from_head = first || c_lo - ka.halo < ka.nhs;      // (a span shorter than a halo: the second workgroup starts behind the head too -- see k_smooth_one)
    const long long s0 = from_head ? ka.nhs : c_lo - ka.halo;
    const long long tile_t0 = s0 + (long long)wave * TILE, t0 = tile_t0 + (long long)lane * SUB;
    const bool any_valid = tile_t0 < T && tile_t0 < c_hi + ka.halo;      // (wave-uniform: tiles behind the right-hand halo have nothing to do)
    if (first && wave == NW - 1 && ka.head_in != nullptr)      // the head's observations to the host, first thing
        send_head_in(ka.head_in, ka.head_in_flag, ka.seq, ka.y, ka.nhs, lane);
    build_power_table<D, NW>(ka.P, sPw, lane, wave);
    // ---- forward, zero start
    double u[SUB], x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) u[j] = 0.0;
    if (any_valid) {
        load_lane_obs<SUB>(ka.y, t0, T, ka.hh, u);
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            double nx[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double v = fma(ka.kA[i], u[j], ka.a[i]);
#pragma unroll
                for (int k = 0; k < D; ++k) v = fma(ka.Phi[i][k], x[k], v);
                nx[i] = v;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) x[i] = nx[i];
        }
    }
    __syncthreads();
    double st[D];
    if (any_valid) scan_forward<D>(ka.P, sPw, lane, x);
    end_forward<D>(x, any_valid, lane, sF[wave], st);
    __syncthreads();
    // ---- the true start state, then the lane's predicted means and innovations
    double mus[SUB][D], r[SUB], psi[D];
#pragma unroll
    for (int i = 0; i < D; ++i) psi[i] = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
        r[j] = 0.0;
#pragma unroll
        for (int i = 0; i < D; ++i) mus[j][i] = 0.0;
    }
    if (any_valid) {
        double mu0v[D];
#pragma unroll
        for (int i = 0; i < D; ++i) mu0v[i] = ka.mu0[i];
        if (from_head && wave < 3 && ka.mu0_flag != nullptr) {      // (wave-uniform) the head's end state comes from the host, beside the kernel
            wait_tables(ka.mu0_flag, ka.seq, &sPoison);
#pragma unroll
            for (int i = 0; i < D; ++i) mu0v[i] = ka.mu0p[i];
        }
        chain_forward<D, NW>(ka.PT, sF, sPw, wave, lane, from_head, mu0v, st);
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            double rr = u[j];
#pragma unroll
            for (int k = 0; k < D; ++k) {
                mus[j][k] = st[k];
                rr = fma(-ka.h[k], st[k], rr);
            }
            r[j] = t0 + j < T ? rr : 0.0;      // (steps behind the series' end: no innovation, no adjoint)
            double nx[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double v = fma(ka.kA[i], u[j], ka.a[i]);
#pragma unroll
                for (int k = 0; k < D; ++k) v = fma(ka.Phi[i][k], st[k], v);
                nx[i] = v;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) st[i] = nx[i];
        }
        // ---- backward, zero psi behind the lane: psi <- Phi' psi + h r / S
#pragma unroll
        for (int j = SUB - 1; j >= 0; --j) {
            const double c = r[j] * ka.iS;
            double np[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double v = ka.h[i] * c;
#pragma unroll
                for (int k = 0; k < D; ++k) v = fma(ka.Phi[k][i], psi[k], v);
                np[i] = v;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) psi[i] = np[i];
        }
        // reverse scan: lane l <- sum_{m >= l} (Phi')^(8 (m - l)) psi_m
        scan_backward<D, true>(ka.P, sPw, lane, psi);
    }
    double pin[D];      // the adjoint behind the lane's last step
    end_backward<D>(psi, any_valid, lane, sB[wave], pin);
    __syncthreads();
    double acc[NS];
#pragma unroll
    for (int e = 0; e < NS; ++e) acc[e] = 0.0;
    if (any_valid) {
        double zin[D];
        chain_backward<D, NW, true>(ka.PT, sB, sPw, wave, lane, zin, pin);
        // ---- the last sweep: the lane's steps backwards with the true adjoint; sums over the steps the workgroup owns
#pragma unroll
        for (int j = SUB - 1; j >= 0; --j) {
            const long long t = t0 + j;
            const double own = (t >= c_lo && t < c_hi) ? 1.0 : 0.0;
            const double rj = r[j];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const double pw = pin[i] * own;
#pragma unroll
                for (int k = 0; k < D; ++k) acc[i * D + k] = fma(pw, mus[j][k], acc[i * D + k]);
                acc[D * D + i] += pw;
                acc[D * D + D + i] = fma(pw, rj, acc[D * D + D + i]);
                acc[D * D + 2 * D + i] = fma(rj * own, mus[j][i], acc[D * D + 2 * D + i]);
            }
            acc[D * D + 3 * D] = fma(rj, own, acc[D * D + 3 * D]);
            acc[D * D + 3 * D + 1] = fma(rj * own, rj, acc[D * D + 3 * D + 1]);
            const double c = rj * ka.iS;
            double np[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double v = ka.h[i] * c;
#pragma unroll
                for (int k = 0; k < D; ++k) v = fma(ka.Phi[k][i], pin[k], v);
                np[i] = v;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) pin[i] = np[i];
        }
        if (first && wave == 0 && lane == 0) {
#pragma unroll
            for (int i = 0; i < D; ++i) ka.psi_out[i] = pin[i];      // d logpdf / d mu at step nhs: where the host's half takes over
        }
    }
#pragma unroll
    for (int e = 0; e < NS; ++e) {
        const double s = wave_sum_to_lane63(acc[e]);
        if (lane == 63) sAcc[wave][e] = s;
    }
    __syncthreads();
    if (threadIdx.x < NS) {
        double tsum = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) tsum += sAcc[w][threadIdx.x];
        ka.part[g * NS + threadIdx.x] = tsum + sPoison;      // (NaN once a bounded wait for the host ran out: the call's result is discarded)
    }
}

template <int D>
int launch_adjoint(hipStream_t st, const tgp_plan::FilterPlan& fp, const double* mu0, const double* y, long long T, double* part, double* psi_out, const HeadHandover* hh) {
    GArgs<D> ka;
    static_assert(sizeof(GArgs<D>) <= 4096, "the kernel-argument segment");
    std::memset(&ka, 0, sizeof ka);
    for (int i = 0; i < D; ++i) {
        ka.a[i] = fp.a[i];
        ka.kA[i] = fp.kA[i];
        ka.h[i] = fp.h[i];
        ka.mu0[i] = mu0 != nullptr ? mu0[i] : 0.0;
        for (int k = 0; k < D; ++k) ka.Phi[i][k] = fp.Phi[i * D + k];
    }
    fill_powers<D>(ka.P, ka.PT, fp.P, fp.PT);
    ka.hh = fp.hh;
    ka.iS = fp.iS;
    ka.T = T;
    ka.nhs = fp.nhs;
    ka.halo = fp.halo;
    ka.C = adjoint_span(fp);
    ka.nwg = adjoint_workgroups(fp, T);
    ka.y = y;
    ka.part = part;
    ka.psi_out = psi_out;
    if (hh != nullptr) {
        ka.head_in = hh->head_in;
        ka.head_in_flag = hh->head_in_flag;
        ka.mu0p = hh->mu0;
        ka.mu0_flag = hh->mu0_flag;
        ka.seq = hh->seq;
    }
    return launch_spans(k_adjoint_one<D, kNW>, ka.nwg, st, ka);
}
}  // namespace

long long adjoint_span(const tgp_plan::FilterPlan& fp) { return (long long)kNW * 64 * kWJ - 2LL * fp.halo; }
long long adjoint_workgroups(const tgp_plan::FilterPlan& fp, long long T) {
    const long long C = adjoint_span(fp);
    return C > 0 ? (T - fp.nhs + C - 1) / C : -1;
}

int adjoint_lti(hipStream_t stream, const tgp_plan::FilterPlan& fp, const double* mu_start, const double* y, long long T, double* part, double* psi_out,
                const HeadHandover* hh) {
    return dispatch_d<kAdjointMaxD>(fp.d, [&](auto d) { return launch_adjoint<decltype(d)::value>(stream, fp, mu_start, y, T, part, psi_out, hh); });
}

// =================================================================================================================================
// logpdf + posterior marginals of an LTI model behind its head on DENSE powers in BOTH directions (round 5): the models the modal
// plan declines (a defective closed loop: two summands with one length scale, ...).  k_adjoint_one's skeleton -- spans with a halo at both ends,
// forward sweep from zero + DPP scan on the powers of Phi, reverse sweep from zero + reverse DPP scan, tiles chained through LDS -- with the
// smoother's recursion in the innovations going backwards, xi_t = c r_t + G xi_(t+1), on the powers of G (a second per-lane table), and no
// second sweep in either direction: the lane's true start state reaches its innovations through the rows h' Phi^j, its right-hand xi reaches
// its outputs through the rows h' G^(7-j) (the WJ / WG trick of k_steady_one, dense).  mean_t = y_t - (R/S) r_t + h' xi_(t+1);
// var_t = h' Ps h + R_new (constant but for the last n1 steps: tvb, pinned host memory, read in place by the last tiles).
// =================================================================================================================================
namespace {
template <int D>
struct SArgs {
    double Phi[D][D], a[D], kA[D], h[D], hh, rS, vb;
    double P[6][D][D], PT[2][D][D];
    double G[D][D], c[D];
    double GP[6][D][D], GPT[2][D][D];
    double WJ[kWJ][D], WG[kWJ][D];
    double mu0[D];
    long long T, C, nwg, nhs, n1;
    int halo, halo_r, rnew_per_step;      // halo_r: the halo behind a span (0 without the backward half)
    const double *y, *Rnew, *tvb;
    double *mean, *var, *part, *xi_out;
    // the head beside the kernel (tgp_powers.hpp SmoothCall): all pinned host memory, flags hold 2 seq once raised
    const double* mu0p;
    const long long* mu0_flag;
    long long* xi_flag;
    double* head_in;
    long long* head_in_flag;
    const double* head_out;
    const long long* head_out_flag;
    long long seq;
    // RAND: a draw from the posterior instead of its marginals (lgssm.jl:65-91 on the reverse-time model of :193-221).  With delta_t = x_t - m_t the
    // reverse-time step x_(t-1) = G x_t + g_t + U' eps_t is the smoother's recursion with a noise input: xi_t = c r_t + G xi_(t+1) + U' eps_t,
    // y_t = y_obs_t - (R / S) r_t + h' xi_(t+1) + sqrt(Rnew_t) eta_t.  U: the upper Cholesky factor of the settled L + 1e-9 I (U[k][i], k <= i);
    // xi_T = U0' eps_0 (the draw of the final filtering state) enters step T - 1 as v0 = G xi_T and its output as s0 = h' xi_T.
    const double* hhT;      // the emission offset per step (a mean function at the inputs, lti_sde.jl:118-131), or nullptr: hh above.  The gains do not see it.
    const double *eps_t, *eps_e;
    static constexpr int RD = D <= kSmoothRandMaxD ? D : 1;      // (the kernel-argument segment is full at d = 8: no room for what d > 4 never uses)
    double U[RD][RD], v0[RD], s0;
};

template <int D, int NW, int MINW, bool RAND>
__global__ __launch_bounds__(NW * 64, MINW) void k_smooth_one(const SArgs<D> by_value) {      // (RAND: `mean` receives the draw, `var` is unused)
    (void)by_value;
    const SArgs<D>& ka = *(const SArgs<D>*)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int SUB = kWJ, TILE = 64 * SUB;
    __shared__ double sF[NW][D], sB[NW][D], sAcc[NW];
    __shared__ double sPw[D][D][64];       // Phi^(8 e), e = 0 .. 63
    __shared__ double sPg[D][D][64];       // G^(8 e)
    __shared__ double sPoison;             // NaN once a bounded wait ran out (wait_tables): the call's result is then discarded
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) sPoison = 0.0;
    long long g;
    if (!span_of_block(ka.nwg, &g)) return;
    const long long T = ka.T, c_lo = ka.nhs + g * ka.C, c_hi = (c_lo + ka.C < T) ? c_lo + ka.C : T;
    const bool first = g == 0;
    // a workgroup whose run-in would reach back into the head (a span shorter than a halo: the second workgroup) starts behind the head like the
    // first, from the head's exact end state: its tiles still cover its range and the halo behind it
    const bool from_head = first || c_lo - ka.halo < ka.nhs;
    const long long s0 = from_head ? ka.nhs : c_lo - ka.halo;
    const long long tile_t0 = s0 + (long long)wave * TILE, t0 = tile_t0 + (long long)lane * SUB;
    const bool any_valid = tile_t0 < T && tile_t0 < c_hi + ka.halo_r;      // (wave-uniform: tiles behind the right-hand halo have nothing to do)
    if (first && wave == NW - 1 && ka.head_in != nullptr) {      // the head's inputs to the host, first thing: its forward recursion runs there
        if (ka.mean != nullptr) {      // its new noise variances, behind y
            if (ka.rnew_per_step) {
                for (long long t = lane; t < ka.nhs; t += 64) ka.head_in[ka.nhs + t] = ka.Rnew[t];
            } else if (lane == 0) {
                ka.head_in[ka.nhs] = ka.Rnew[0];
            }
        }
        if constexpr (RAND) {      // the head's draws: eta [nhs] behind y | Rnew, then eps [nhs][D]
            for (long long t = lane; t < ka.nhs; t += 64) ka.head_in[2 * ka.nhs + t] = ka.eps_e[t];
            for (long long e = lane; e < ka.nhs * D; e += 64) ka.head_in[3 * ka.nhs + e] = ka.eps_t[e];
        }
        if (ka.hhT != nullptr) {      // the head's emission offsets, behind everything else (offset 10 nhs)
            for (long long t = lane; t < ka.nhs; t += 64) ka.head_in[10 * ka.nhs + t] = ka.hhT[t];
        }
        send_head_in(ka.head_in, ka.head_in_flag, ka.seq, ka.y, ka.nhs, lane);
    }
    // ---- the observations first (they are on their way while the tables are built)
    double u[SUB];
#pragma unroll
    for (int j = 0; j < SUB; ++j) u[j] = 0.0;
    if (any_valid) {
        if (ka.hhT != nullptr) {      // (kernel-uniform) an emission offset per step
#pragma unroll
            for (int j = 0; j < SUB; ++j) u[j] = t0 + j < T ? ka.y[t0 + j] - ka.hhT[t0 + j] : 0.0;
        } else {
            load_lane_obs<SUB>(ka.y, t0, T, ka.hh, u);
        }
    }
    {   // the per-lane power tables of Phi and -- with the backward half -- of G, the 2 D rows dealt over the waves (the stores stand here, on
        // the arrays themselves: through a shared block's references k_smooth_one<6, 8, 4, false> spills 80 bytes instead of 64)
        const int uw = __builtin_amdgcn_readfirstlane(wave);
#pragma unroll
        for (int i2 = 0; i2 < 2 * D; ++i2) {
            if (uw != i2 % NW) continue;
            const int i = i2 % D;
            const bool isg = i2 >= D;
            if (isg && ka.mean == nullptr) continue;      // (logpdf only: no backward half)
            double row[D];
            if (isg) {
                power_row<D>(ka.GP, i, lane, row);
#pragma unroll
                for (int k = 0; k < D; ++k) sPg[i][k][lane] = row[k];
            } else {
                power_row<D>(ka.P, i, lane, row);
#pragma unroll
                for (int k = 0; k < D; ++k) sPw[i][k][lane] = row[k];
            }
        }
    }
    // ---- forward, zero start: the lane's innovations r0 and its end state
    double r[SUB], x[D];
#pragma unroll
    for (int i = 0; i < D; ++i) x[i] = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) r[j] = 0.0;
    if (any_valid) {
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            double rr = u[j];
#pragma unroll
            for (int k = 0; k < D; ++k) rr = fma(-ka.h[k], x[k], rr);
            r[j] = rr;
            double nx[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                double v = fma(ka.kA[i], u[j], ka.a[i]);
#pragma unroll
                for (int k = 0; k < D; ++k) v = fma(ka.Phi[i][k], x[k], v);
                nx[i] = v;
            }
#pragma unroll
            for (int i = 0; i < D; ++i) x[i] = nx[i];
        }
    }
    __syncthreads();
    double st[D];
    if (any_valid) scan_forward<D>(ka.P, sPw, lane, x);
    end_forward<D>(x, any_valid, lane, sF[wave], st);
    __syncthreads();
    // ---- the true start state -> the true innovations (r = r0 - h' Phi^j st); the reverse sweep from zero
    double xi[D], o0[SUB], acc = 0.0;
#pragma unroll
    for (int i = 0; i < D; ++i) xi[i] = 0.0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) o0[j] = 0.0;
    if (any_valid) {
        double mu0v[D];
#pragma unroll
        for (int i = 0; i < D; ++i) mu0v[i] = ka.mu0[i];
        if (from_head && wave < 3 && ka.mu0_flag != nullptr) {      // (wave-uniform) the head's end state comes from the host, beside the kernel
            wait_tables(ka.mu0_flag, ka.seq, &sPoison);
#pragma unroll
            for (int i = 0; i < D; ++i) mu0v[i] = ka.mu0p[i];
        }
        chain_forward<D, NW>(ka.PT, sF, sPw, wave, lane, from_head, mu0v, st);
#pragma unroll
        for (int j = 0; j < SUB; ++j) {
            double rr = r[j];
#pragma unroll
            for (int k = 0; k < D; ++k) rr = fma(-ka.WJ[j][k], st[k], rr);
            const long long t = t0 + j;
            rr = t < T ? rr : 0.0;      // (steps behind the series' end: no innovation)
            r[j] = rr;
            if (t >= c_lo && t < c_hi) acc = fma(rr, rr, acc);
            // h' m_t + hh_t = y_t - (R / S) r_t: what the smoother adds h' xi_(t+1) to  (a per-step offset is fetched again: the L2 has it)
            o0[j] = fma(-ka.rS, rr, u[j] + ((ka.hhT != nullptr && t < T) ? ka.hhT[t] : ka.hh));
        }
        if (ka.mean != nullptr) {
            double ee[RAND ? SUB : 1][RAND ? D : 1];      // (RAND) the lane's transition draws: 8 D consecutive doubles of eps_t
            if constexpr (RAND) {
#pragma unroll
                for (int j = 0; j < SUB; ++j)
#pragma unroll
                    for (int k = 0; k < D; ++k) ee[j][k] = (t0 + j < T) ? ka.eps_t[(t0 + j) * D + k] : 0.0;
            }
#pragma unroll
            for (int j = SUB - 1; j >= 0; --j) {
                double o = o0[j];
#pragma unroll
                for (int k = 0; k < D; ++k) o = fma(ka.h[k], xi[k], o);
                o0[j] = o;
                double np[D];
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    double v = ka.c[i] * r[j];
#pragma unroll
                    for (int k = 0; k < D; ++k) v = fma(ka.G[i][k], xi[k], v);
                    if constexpr (RAND) {      // + (U' eps)_i; the series' last step also takes G xi_T
#pragma unroll
                        for (int k = 0; k <= i; ++k) v = fma(ka.U[k][i], ee[j][k], v);
                        if (t0 + j == T - 1) v += ka.v0[i];
                    }
                    np[i] = v;
                }
#pragma unroll
                for (int i = 0; i < D; ++i) xi[i] = np[i];
            }
            // reverse scan: lane l <- sum_{m >= l} G^(8 (m - l)) xi_m
            scan_backward<D, false>(ka.GP, sPg, lane, xi);
        }
    }
    if (ka.mean != nullptr) {      // (kernel-uniform)
        double pin[D];      // xi behind the lane's last step
        end_backward<D>(xi, any_valid, lane, sB[wave], pin);
        __syncthreads();
        if (any_valid) {
            double zin[D];
            chain_backward<D, NW, false>(ka.GPT, sB, sPg, wave, lane, zin, pin);
            if (first && wave == 0 && lane == 0) {      // xi at step nhs: where the host's half takes over (G^512 zin + the tile's own)
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    double v = xi[i];
#pragma unroll
                    for (int k = 0; k < D; ++k) v = fma(ka.GPT[0][i][k], zin[k], v);
                    ka.xi_out[i] = v;
                }
                if (ka.xi_flag != nullptr) {
                    __threadfence_system();
                    __hip_atomic_store(ka.xi_flag, 2 * ka.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
                }
            }
            // ---- outputs of the steps the workgroup owns
            const bool whole = t0 >= c_lo && t0 + SUB <= c_hi;
            const bool al = ((reinterpret_cast<uintptr_t>(ka.mean) | (RAND ? (uintptr_t)0 : reinterpret_cast<uintptr_t>(ka.var))) & 15) == 0;
            const double rn0 = ka.rnew_per_step ? 0.0 : ka.Rnew[0];
            const bool in_tail = t0 + SUB > T - ka.n1;
            const bool wide = whole && al;      // (t0 is a multiple of 8: spans start on multiples of 16 behind nhs, itself one)
#pragma unroll
            for (int j2 = 0; j2 < SUB; j2 += 2) {
                double om[2], ov[2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    const int j = j2 + jj;
                    const long long t = t0 + j;
                    double o = o0[j];
#pragma unroll
                    for (int k = 0; k < D; ++k) o = fma(ka.WG[j][k], pin[k], o);
                    double v = 0.0;
                    if constexpr (RAND) {      // the draw: + h' xi_T at the series' last step, + sqrt(Rnew_t) eta_t
                        if (t == T - 1) o += ka.s0;
                        if (t < T) o = fma(sqrt(ka.rnew_per_step ? ka.Rnew[t] : rn0), ka.eps_e[t], o);
                    } else {
                        v = ka.vb;
                        if (in_tail && t < T && T - 1 - t < ka.n1) v = ka.tvb[T - 1 - t];
                        if (ka.rnew_per_step) v += (t < T ? ka.Rnew[t] : 0.0);
                        else v += rn0;
                    }
                    om[jj] = o;
                    ov[jj] = v;
                }
                if (wide) {
                    v2d w;
                    w.x = om[0];
                    w.y = om[1];
                    reinterpret_cast<v2d*>(ka.mean + t0)[j2 / 2] = w;
                    if constexpr (!RAND) {
                        w.x = ov[0];
                        w.y = ov[1];
                        reinterpret_cast<v2d*>(ka.var + t0)[j2 / 2] = w;
                    }
                } else {
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const long long t = t0 + j2 + jj;
                        if (t >= c_lo && t < c_hi) {
                            ka.mean[t] = om[jj];
                            if constexpr (!RAND) ka.var[t] = ov[jj];
                        }
                    }
                }
            }
        }
    }
    if (ka.head_out_flag != nullptr && ka.mean != nullptr && g == ((ka.nwg + 7) / 8) / 2) {      // the head's outputs, by a workgroup from the middle of the dispatch (see k_steady_one)
        if (wave < (RAND ? 1 : 2)) {
            wait_tables(ka.head_out_flag, ka.seq, &sPoison);
            double* dst = wave == 0 ? ka.mean : ka.var;
            const double* src = ka.head_out + (wave == 0 ? 0 : ka.nhs);
            for (long long t = lane; t < ka.nhs; t += 64) dst[t] = src[t];
        }
    }
    acc = wave_sum_to_lane63(acc);
    if (lane == 63) sAcc[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double tsum = 0.0;
#pragma unroll
        for (int w = 0; w < NW; ++w) tsum += sAcc[w];
        ka.part[g] = tsum + sPoison;
    }
}

template <int D>
int launch_smooth(hipStream_t st, const tgp_plan::SmoothPlan& sp, const double* mu0, const SmoothCall& c) {
    const tgp_plan::FilterPlan& fp = sp.fp;
    SArgs<D> ka;
    static_assert(sizeof(SArgs<D>) <= 11264, "the kernel-argument segment (12 KB launch on gfx950: scripts/micro/bigarg.hip)");
    std::memset(&ka, 0, sizeof ka);
    for (int i = 0; i < D; ++i) {
        ka.a[i] = fp.a[i];
        ka.kA[i] = fp.kA[i];
        ka.h[i] = fp.h[i];
        ka.c[i] = sp.c[i];
        ka.mu0[i] = mu0 != nullptr ? mu0[i] : 0.0;
        for (int j = 0; j < kWJ; ++j) {
            ka.WJ[j][i] = sp.WJ[j][i];
            ka.WG[j][i] = sp.WG[j][i];
        }
        for (int k = 0; k < D; ++k) {
            ka.Phi[i][k] = fp.Phi[i * D + k];
            ka.G[i][k] = sp.G[i * D + k];
        }
    }
    fill_powers<D>(ka.P, ka.PT, fp.P, fp.PT);
    fill_powers<D>(ka.GP, ka.GPT, sp.GP, sp.GPT);
    ka.hh = fp.hh;
    ka.rS = sp.rS;
    ka.vb = sp.vb;
    ka.T = c.T;
    ka.nhs = fp.nhs;
    ka.n1 = sp.n1;
    const bool post = c.mean != nullptr;
    ka.halo = sp.halo;
    ka.halo_r = post ? sp.halo : 0;
    ka.C = smooth_span(sp, post);
    ka.nwg = smooth_workgroups(sp, c.T, post);
    ka.rnew_per_step = c.rnew_per_step;
    ka.y = c.y;
    ka.Rnew = c.Rnew;
    ka.tvb = c.tvb;
    ka.mean = c.mean;
    ka.var = c.var;
    ka.part = c.part;
    ka.xi_out = c.xi_out;
    ka.hhT = c.hh_t;
    ka.mu0p = c.mu0;
    ka.mu0_flag = c.mu0_flag;
    ka.xi_flag = c.xi_flag;
    ka.head_in = c.head_in;
    ka.head_in_flag = c.head_in_flag;
    ka.head_out = c.head_out;
    ka.head_out_flag = c.head_out_flag;
    ka.seq = c.seq;
    static const int minw_env = [] { const char* v = std::getenv("TGP_SMOOTH_MINW"); return v ? std::atoi(v) : 0; }();
    const bool four = minw_env ? minw_env >= 4 : D <= 6;
    if (c.eps_t != nullptr) {      // a draw from the posterior (d <= kSmoothRandMaxD: the lane's 8 d draws sit in registers)
        if constexpr (D <= kSmoothRandMaxD) {
            ka.eps_t = c.eps_t;
            ka.eps_e = c.eps_e;
            for (int i = 0; i < D; ++i) {
                ka.v0[i] = c.v0[i];
                for (int k = 0; k < D; ++k) ka.U[i][k] = c.U[i * D + k];
            }
            ka.s0 = c.s0;
            return launch_spans(k_smooth_one<D, kNW, 2, true>, ka.nwg, st, ka);
        } else {
            return (int)hipErrorInvalidValue;
        }
    }
    if (four && D <= 6) return launch_spans(k_smooth_one<D, kNW, (D <= 6 ? 4 : 2), false>, ka.nwg, st, ka);
    return launch_spans(k_smooth_one<D, kNW, 2, false>, ka.nwg, st, ka);
}
}  // namespace

// (sixteen waves per workgroup -- spans of 8192 steps, half the halo overhead, the tables' rows dealt over sixteen waves -- were measured
//  SLOWER: fused call 0.228 against 0.177 ms at d = 6, T = 1e7: one workgroup per CU leaves nothing to run beside its barriers)
long long smooth_span(const tgp_plan::SmoothPlan& sp, bool post) { return (long long)kNW * 64 * kWJ - (post ? 2LL : 1LL) * sp.halo; }
long long smooth_workgroups(const tgp_plan::SmoothPlan& sp, long long T, bool post) {
    const long long C = smooth_span(sp, post);
    return C > 0 ? (T - sp.fp.nhs + C - 1) / C : -1;
}

int smooth_lti(hipStream_t stream, const tgp_plan::SmoothPlan& sp, const double* mu_start, const SmoothCall& c) {
    return dispatch_d<8>(sp.fp.d, [&](auto d) { return launch_smooth<decltype(d)::value>(stream, sp, mu_start, c); });
}

// ---- The host plans other translation units need (tgp_api.hip: the filter / posterior / rand / smooth one-launch paths).  Defined HERE and only
// here: this object's host code is built with -mavx2 -mfma, and the inline functions of tgp_steady_plan.hpp instantiated in an object built
// with other flags would be two definitions of one entity -- the linker keeps either (round-4 advice).  All behind the run-time CPU check: a
// host without AVX2 gets a plan that declines (the older engines serve the call).
void plan_filter(const tgp_plan::ModelHost& m, long long T, tgp_plan::FilterPlan& fp) {
    if (!tgp_modal::host_cpu_ok()) {
        fp.why = tgp_plan::kEigFail;
        return;
    }
    tgp_plan::build_filter_any(m, T, fp);
}
void plan_filter_head(const tgp_plan::ModelHost& m, const tgp_plan::FilterPlan& fp, const double* y, double* mout, double* Pout, double* mu_end, double* quad) {
    tgp_plan::filter_head_any(m, fp, y, mout, Pout, mu_end, quad);      // (only ever called with a plan plan_filter accepted)
}
bool plan_posterior_head(const tgp_plan::ModelHost& m, const tgp_plan::FilterPlan& fp, const double* y, double* Gh, double* gh, double* Lh, double* Gss,
                         double* Lss, double* mu_end, double* quad) {
    return tgp_plan::posterior_head_any(m, fp, y, Gh, gh, Lh, Gss, Lss, mu_end, quad);
}
void plan_rand(const tgp_plan::ModelHost& m, tgp_plan::RandPlan& rp) {
    if (!tgp_modal::host_cpu_ok()) {
        rp.why = tgp_plan::kEigFail;
        return;
    }
    tgp_plan::build_rand_any(m, rp);
}
void plan_smooth(const tgp_plan::ModelHost& m, long long T, tgp_plan::SmoothPlan& sp, double* tvb, bool post) {
    if (!tgp_modal::host_cpu_ok()) {
        sp.why = tgp_plan::kEigFail;
        return;
    }
    tgp_plan::build_smooth_any(m, T, sp, tvb, post);
    // (halos would eat three quarters of a span.  Workgroup g >= 1 starts `halo` steps in front of its range; with a span shorter than a halo that
    //  reaches back into the head -- or in front of the series: a memory fault found by the randomised sweep, T = 250 000, two Matern-1/2 of one
    //  length scale, halo 1520 against spans of 1056.
    //  Such a workgroup -- only the second one can be: 2 spans + a halo fit its tiles exactly when a span is shorter than a halo -- starts behind
    //  the head like the first, from the head's exact end state (`from_head` in the kernels).
    if (sp.why == tgp_plan::kOk && smooth_span(sp, post) < 1024) sp.why = tgp_plan::kSlowMixing;
}
void plan_smooth_head_forward(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp, const double* y, double* mu_end, double* quad, const double* hh_t) {
    tgp_plan::smooth_head_forward_any(m, sp, y, mu_end, quad, hh_t);
}
bool plan_smooth_head_tables(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp) { return tgp_plan::smooth_head_tables_any(m, sp); }
void plan_smooth_head_backward(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp, const double* y, const double* lam, double* mean, double* vb) {
    tgp_plan::smooth_head_backward_any(m, sp, y, lam, mean, vb);
}
bool plan_smooth_rand_factors(const tgp_plan::SmoothPlan& sp, const double* eps0, double* U, double* v0, double* s0) {
    return tgp_plan::smooth_rand_factors_any(sp, eps0, U, v0, s0);
}
void plan_smooth_head_backward_rand(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp, const double* y, const double* delta, const double* eps_e,
                                    const double* eps_t, const double* rn, bool rn_per_step, double* out) {
    tgp_plan::smooth_head_backward_rand_any(m, sp, y, delta, eps_e, eps_t, rn, rn_per_step, out);
}

}  // namespace tgp_powers
