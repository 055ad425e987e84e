// Dense engine, mid-sized states (16 < d <= 64, p <= 16): a draw from posterior(model, y) with replaced observation noise
// (rand(rng, posterior(fx, y)(x_new)), posterior_lti_sde.jl:48-58 -> lgssm.jl:65-91 on the Reverse model of lgssm.jl:193-238) WITHOUT writing that
// model: the reverse-time walk behind the forward pass's stores (m_f, P_f and the per-update records of dk_chunk_filter / dk_fused_filter), one
// 256-thread workgroup walking the steps downwards as fused_smooth_walk does (scripts/dense_chunk_draw_proto.py is the restatement).
//
// The walk carries the deviation from the filtered mean, delta_t = x_t - m_f[t] (the wide engine's form):
//     y*_t        = H_t (m_f[t] + delta_t) + h_t + sqrt(Rnew_t) e_t
//     delta_{t-1} = G_t (delta_t + sum_j v_j nu_j / s_j) + U_t' eps_t[t]
// and per step, from P = P_f[t-1] and the step's A, Q (invert_dynamics, lgssm.jl:231-238, and lgc.jl:84-87):
//     T1 = A P,   Pp = T1 A' + Q                       two MFMA products (fragments of A and the Q tiles as fused_filter_walk holds them)
//     Uc'Uc = Pp + 1e-10 I,   W = Uc'^-1 [T1 | z]      ONE right-looking sweep over the rows of [Pp | T1 | z] in LDS, z = delta_t + (m_t - m^p_t)
//     L = P - W'W                                      MFMA product, in place of P (upper tiles: the factorisation reads the upper triangle, as
//                                                      the reference's Symmetric does)
//     U'U = L + 1e-9 I                                 the same sweep on L
//     delta_{t-1} = W'u + U' eps                       u = Uc'^-1 z is column d of W; G itself is never formed
// fp64 throughout. A pivot that is not positive, or a deviation that is not finite, poisons what the chunk hands to the check (dk_chunk_close, status
// bit 8) / raises the sequential pass's flag.
//
// Included by tgp_dense.hip behind tgp_dense_chunked.hpp (namespace tgp_dense).
#pragma once

struct FusedDrawArgs {
    int64_t T = 0;
    int64_t step0 = 0, step1 = 0;      // time steps [step0, step1) of this launch, walked from step1 - 1 down to step0
    int d = 0, p = 0, Pq = 0, small_out = 0;
    const double *A = nullptr, *Q = nullptr, *H = nullptr, *h = nullptr;      // padded blocks (tgp_dense.hip layouts)
    int64_t sA = 0, sQ = 0, sH = 0, sh = 0;
    const double* m_f = nullptr;       // [T][d] filtering means
    const double* P_f = nullptr;       // [T][d*d] filtering covariances (column-major)
    const double* aux = nullptr;       // [T][p][d + 2] records (v, s, nu) of the forward pass
    const double* Rnew = nullptr;      // [T][p] or [p]
    int64_t sRn = 0;
    const double* eps_t = nullptr;     // [T][d]: row t drives the transition out of step t
    const double* eps_e = nullptr;     // [T][p]
    const double* d0 = nullptr;        // [DP] delta of step step1 - 1 (null: zero -- a chunk's warm-up)
    double* dout = nullptr;            // [DP] delta of step step0 - 1 (step0 > 0), what the next launch / the neighbour's check takes
    double* y_out = nullptr;           // [T][p]
    double* stat = nullptr;            // sequential pass: [0] = 1 when a pivot was not positive, 2 when the deviation left the launch non-finite
};

template <int DP>
struct FusedDrawCfg {
    static constexpr int NT = DP / 16, KS = DP / 4, LD = DP + 4, LD2 = 2 * LD, NG = 256 / DP;
    static constexpr int ZC = LD + DP;                        // column of z in a row of [Pp | T1 | z]
    static constexpr int NQ2 = (ZC + 1 + 63) / 64;            // columns per lane in the sweep over [Pp | T1 | z]
    // LDS (doubles): [Pp -> Uc | T1 -> W | z -> u] | P -> L -> U | delta | m_f | eps | partial sums | H rows | scalars | records
    static constexpr int oST = 0, oP = oST + DP * LD2, oD = oP + DP * LD, oM = oD + DP, oE = oM + DP, oRed = oE + DP, oH = oRed + NG * DP,
                         oS = oH + 16 * DP, oAux = oS + 64, TOTAL = oAux + 16 * (DP + 2);
    static constexpr int APT = (16 * (DP + 2) + 255) / 256;      // record values per thread (prefetch registers)
    static constexpr size_t LDS_BYTES = (size_t)TOTAL * sizeof(double);
};
// (one workgroup per CU at DP = 64 within the 160 KiB; tests/test_dense_chunk_draw_resources.py restates the counts)
static_assert(FusedDrawCfg<32>::LDS_BYTES == 39424 && FusedDrawCfg<48>::LDS_BYTES == 76032 && FusedDrawCfg<64>::LDS_BYTES == 125184, "FusedDrawCfg: LDS layout");
static_assert(FusedDrawCfg<64>::LDS_BYTES <= 160 * 1024, "FusedDrawCfg: LDS per CU");

// In-place upper Cholesky of the leading DP x DP block of M (row stride LDM; only the upper triangle is read and written), right-looking by rows, with the
// columns [XC0, XC1) of every row riding along as right-hand sides of U'^-1: afterwards row k holds U[k][k..] and (U'^-1 X)[k][.].
// One barrier per row: wave 0 finishes row k + 1 (its pivot included) in the same pass that updates it. NQ columns per lane (col = lane + 64 q).
template <int DP, int LDM, int XC0, int XC1, int NQ>
__device__ __forceinline__ void chol_sweep(double* M, int lane, int w, double* badflag) {
    auto live = [&](int col, int i) { return (col >= i && col < DP) || (col >= XC0 && col < XC1); };
    if (w == 0) {      // row 0
        double x[NQ];
#pragma unroll
        for (int q = 0; q < NQ; ++q) x[q] = live(lane + 64 * q, 0) ? M[lane + 64 * q] : 0.0;
        const double piv = rdlane(x[0], 0);
        if (!(piv > 0.0) && lane == 0) *badflag = 1.0;
        const double rinv = 1.0 / sqrt(piv);
#pragma unroll
        for (int q = 0; q < NQ; ++q)
            if (live(lane + 64 * q, 0)) M[lane + 64 * q] = x[q] * rinv;
    }
    lds_barrier();
    for (int k = 0; k + 1 < DP; ++k) {
        double rk[NQ];
        const double* Mk = M + k * LDM;
#pragma unroll
        for (int q = 0; q < NQ; ++q) rk[q] = live(lane + 64 * q, k + 1) ? Mk[lane + 64 * q] : 0.0;
        for (int i = k + 1 + w; i < DP; i += 4) {
            const double ui = Mk[i];
            double* Mi = M + i * LDM;
            double x[NQ];
#pragma unroll
            for (int q = 0; q < NQ; ++q) x[q] = live(lane + 64 * q, i) ? fma(-ui, rk[q], Mi[lane + 64 * q]) : 0.0;
            if (i == k + 1) {      // (wave 0, uniformly) the row the next pass divides by: finish it now
                const double piv = rdlane(x[0], i);
                if (!(piv > 0.0) && lane == 0) *badflag = 1.0;
                const double rinv = 1.0 / sqrt(piv);
#pragma unroll
                for (int q = 0; q < NQ; ++q) x[q] *= rinv;
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
                if (live(lane + 64 * q, i)) Mi[lane + 64 * q] = x[q];
        }
        lds_barrier();
    }
}

// CH = true (dk_chunk_draw): the workgroup owns the steps [step0, run.own0) and walks [run.own0, step1) behind them first, from d0 (the chunk that starts at
// the end of the series) or zero, as a warm-up that writes nothing.
template <int DP, bool CH>
__device__ __forceinline__ void fused_draw_walk(const FusedDrawArgs& g, const FusedChunkRun& run) {
    using C = FusedDrawCfg<DP>;
    constexpr int NT = C::NT, KS = C::KS, LD = C::LD, LD2 = C::LD2, NG = C::NG, ZC = C::ZC, APT = C::APT;
    constexpr int NGW = 4 / NT > 0 ? 4 / NT : 1;       // waves per block index, tiles per wave: as fused_filter_walk
    constexpr int XPW = (NT + NGW - 1) / NGW;
    extern __shared__ double lds[];
    double* sST = lds + C::oST;        // row i: Pp[i][0 .. DP) | pad | T1[i][0 .. DP) at LD | z[i] at ZC
    double* sP = lds + C::oP;
    double* sd = lds + C::oD;
    double* smf = lds + C::oM;
    double* se = lds + C::oE;
    double* red = lds + C::oRed;
    double* sH = lds + C::oH;
    double* ss = lds + C::oS;          // [8] a pivot was not positive; [9] delta not finite; [16..31] h; [32..47] Rnew; [48..63] e of the step
    double* sAux = lds + C::oAux;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lr = lane & 15, lq = lane >> 4;
    const int b = w % NT, grp = w / NT;
    const bool mfma_wave = w < NT * NGW;
    const int d = g.d;
    const int naux = g.p * (d + 2);
    const bool H_shared = g.sH == 0 && g.sh == 0;

    for (int e = tid; e < C::TOTAL; e += 256) lds[e] = 0.0;
    __syncthreads();
    if (tid < DP && g.d0) sd[tid] = g.d0[tid];
    double af[KS];                // A fragments of block row b: af[ks] = A[16 b + lr][4 ks + lq]
    double qf[XPW][4];            // Q tiles (x, b) of this wave
    auto load_A = [&](const double* A) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) af[ks] = A[(b * 16 + lr) + (int64_t)(ks * 4 + lq) * DP];
    };
    auto load_Q = [&](const double* Q) __attribute__((always_inline)) {
#pragma unroll
        for (int x = 0; x < NT; ++x)
            if (x % NGW == grp) {
#pragma unroll
                for (int r = 0; r < 4; ++r) qf[x / NGW][r] = Q[(x * 16 + lq + 4 * r) + (int64_t)(b * 16 + lr) * DP];
            }
    };
    auto load_H = [&](int64_t t) __attribute__((always_inline)) {
        const double* H = g.H + t * g.sH;
        for (int e = tid; e < g.p * DP; e += 256) sH[e] = H[(e / DP) + (int64_t)(e % DP) * g.Pq];
        if (tid < g.p) ss[16 + tid] = g.h[t * g.sh + tid];
    };
    if (g.sA == 0) load_A(g.A);
    if (g.sQ == 0) load_Q(g.Q);
    if (H_shared) load_H(0);
    // the stores of the next (earlier) step travel one step ahead in registers: P_f[t - 1], the records, draws and filtering mean of step t
    constexpr int PPT = (DP * DP) / 256;
    double pf_n[PPT];
    double ax_n[APT];
    double mf_n = 0.0, et_n = 0.0, rn_n = 0.0, ee_n = 0.0;
#pragma unroll
    for (int u = 0; u < PPT; ++u) pf_n[u] = 0.0;      // (step 0 has no P_f[t - 1]: nothing reads what it stages)
    auto fetch = [&](int64_t t) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < APT; ++u) {
            const int e = tid + u * 256;
            ax_n[u] = e < naux ? g.aux[t * (int64_t)naux + e] : 0.0;
        }
        if (tid < DP) et_n = tid < d ? g.eps_t[t * d + tid] : 0.0;
        if (t > 0) {
            const double* P = g.P_f + (t - 1) * (int64_t)d * d;
#pragma unroll
            for (int u = 0; u < PPT; ++u) {
                const int e = tid + u * 256, i = e % DP, j = e / DP;
                pf_n[u] = (i < d && j < d) ? P[i + (int64_t)j * d] : 0.0;
            }
        }
        if (CH && t >= run.own0) return;      // (a warm-up step emits nothing)
        if (tid < DP) mf_n = tid < d ? g.m_f[t * d + tid] : 0.0;
        if (tid < g.p) {
            rn_n = g.Rnew[g.sRn ? t * g.p + tid : tid];
            ee_n = g.eps_e[t * g.p + tid];
        }
    };
    fetch(g.step1 - 1);
    __syncthreads();

    for (int64_t t = g.step1 - 1; t >= g.step0; --t) {
        const bool own = !CH || t < run.own0;
        if constexpr (CH) {
            if (t == run.own0 - 1 && g.step1 > run.own0) {      // the warm-up's end state (sd is complete behind the loop's last barrier)
                if (tid < DP) run.warm[tid] = sd[tid];
            }
        }
        // ---- the stores of step t -> LDS; prefetch step t - 1
#pragma unroll
        for (int u = 0; u < PPT; ++u) {
            const int e = tid + u * 256;
            sP[(e % DP) * LD + e / DP] = pf_n[u];
        }
#pragma unroll
        for (int u = 0; u < APT; ++u) {
            const int e = tid + u * 256;
            if (e < naux) sAux[e] = ax_n[u];
        }
        if (tid < DP) {
            smf[tid] = mf_n;
            se[tid] = et_n;
        }
        if (tid < g.p) {
            ss[32 + tid] = rn_n;
            ss[48 + tid] = ee_n;
        }
        if (t > g.step0) fetch(t - 1);
        if (!H_shared && own) load_H(t);
        lds_barrier();
        // ---- emissions of step t: wave j % 4, lanes over the state
        if (own) {
            for (int j = w; j < g.p; j += 4) {
                double acc = 0.0;
                if (lane < DP) acc = sH[j * DP + lane] * (smf[lane] + sd[lane]);
                const double hx = wave_sum(acc);
                if (lane == 0) {
                    const double Rv = ss[32 + j];
                    g.y_out[t * g.p + j] = hx + ss[16 + j] + sqrt(g.small_out ? Rv + 1e-9 : Rv) * ss[48 + j];
                }
            }
        }
        if (t == 0) break;       // the transition out of step 0 moves to a step nobody emits
        // ---- z = delta_t + (m_t - m^p_t): the step's scalar updates v nu / s from the records (nu = 0 at a missing entry)
        if (tid < DP) {
            double z = sd[tid];
            if (tid < d)
                for (int j = 0; j < g.p; ++j) {
                    const double* ax = sAux + j * (d + 2);
                    z = fma(ax[tid], ax[d + 1] / ax[d], z);
                }
            sST[tid * LD2 + ZC] = z;
        }
        // ---- T1 = A P: tiles (b, x) -> sST[.][LD ..]
        if (g.sA != 0) load_A(g.A + t * g.sA);
        if (g.sQ != 0) load_Q(g.Q + t * g.sQ);
#pragma unroll
        for (int x = 0; x < NT; ++x)
            if (x % NGW == grp && mfma_wave) {
                d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = mfma_f64(af[ks], sP[(ks * 4 + lq) * LD + x * 16 + lr], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) sST[(b * 16 + lq + 4 * r) * LD2 + LD + x * 16 + lr] = acc[r];
            }
        lds_barrier();
        // ---- Pp = T1 A' + Q + 1e-10 I: tiles (x, b) -> sST[.][0 ..]
#pragma unroll
        for (int x = 0; x < NT; ++x)
            if (x % NGW == grp && mfma_wave) {
                d4 acc = d4{qf[x / NGW][0], qf[x / NGW][1], qf[x / NGW][2], qf[x / NGW][3]};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) acc = mfma_f64(sST[(x * 16 + lr) * LD2 + LD + ks * 4 + lq], af[ks], acc);
#pragma unroll
                for (int r = 0; r < 4; ++r) sST[(x * 16 + lq + 4 * r) * LD2 + b * 16 + lr] = acc[r] + ((x == b && lq + 4 * r == lr) ? 1e-10 : 0.0);
            }
        lds_barrier();
        // ---- Uc'Uc = Pp + 1e-10 I, [W | u] = Uc'^-1 [T1 | z]
        chol_sweep<DP, LD2, LD, ZC + 1, C::NQ2>(sST, lane, w, ss + 8);
        // ---- L = P - W'W + 1e-9 I, upper tiles, in place of P
        {
            int idx = 0;
#pragma unroll
            for (int I = 0; I < NT; ++I)
#pragma unroll
                for (int J = I; J < NT; ++J, ++idx)
                    if ((idx & 3) == w) {
                        d4 acc = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
                        for (int ks = 0; ks < KS; ++ks)
                            acc = mfma_f64(sST[(ks * 4 + lq) * LD2 + LD + I * 16 + lr], sST[(ks * 4 + lq) * LD2 + LD + J * 16 + lr], acc);
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            double* pe = sP + (I * 16 + lq + 4 * r) * LD + J * 16 + lr;
                            *pe = (*pe - acc[r]) + ((I == J && lq + 4 * r == lr) ? 1e-9 : 0.0);
                        }
                    }
        }
        lds_barrier();
        // ---- U'U = L + 1e-9 I
        chol_sweep<DP, LD, 0, 0, 1>(sP, lane, w, ss + 8);
        // ---- delta_{t-1} = W'u + U' eps: K-sliced over the threads, summed by the first DP
        {
            const int i = tid % DP, slc = tid / DP;
            if (slc < NG) {
                double s = 0.0;
                for (int k = slc; k < DP; k += NG) {
                    s = fma(sST[k * LD2 + LD + i], sST[k * LD2 + ZC], s);
                    if (k <= i) s = fma(sP[k * LD + i], se[k], s);
                }
                red[slc * DP + i] = s;
            }
            lds_barrier();
            if (tid < DP) {
                double v = 0.0;
#pragma unroll
                for (int q = 0; q < NG; ++q) v += red[q * DP + tid];
                sd[tid] = v;
            }
            lds_barrier();
        }
    }
    __syncthreads();
    if (tid < DP && !(fabs(sd[tid]) <= 1e300)) ss[9] = 1.0;
    __syncthreads();
    const bool badpiv = ss[8] != 0.0, nonfinite = ss[9] != 0.0;
    if constexpr (CH) {
        if (tid < DP) {
            const double nan = __longlong_as_double(0x7ff8000000000000LL);
            g.dout[tid] = (badpiv || nonfinite) ? nan : sd[tid];
            if (badpiv || nonfinite) run.warm[tid] = nan;
        }
    } else {
        if (g.dout && g.step0 > 0 && tid < DP) g.dout[tid] = sd[tid];
        if ((badpiv || nonfinite) && tid == 0) g.stat[0] = badpiv ? 1.0 : 2.0;
    }
}
template <int DP>
__global__ __launch_bounds__(256) void dk_fused_draw(const FusedDrawArgs g) {
    fused_draw_walk<DP, false>(g, FusedChunkRun{});
}

// chunk c owns [c C, min(T, (c + 1) C)), walked downwards from min(T, (c + 1) C + W); `warm` / `fin` hold DP doubles per chunk: delta at the crossing
// into the own steps, and the delta carried out of step c C (the reference of chunk c - 1's warm-up)
template <int DP>
__global__ __launch_bounds__(256) void dk_chunk_draw(const FusedDrawArgs g0, const ChunkGeom q, const double* start) {
    const int64_t c = blockIdx.x;
    FusedDrawArgs g = g0;
    FusedChunkRun run;
    g.step0 = c * q.C;
    run.own0 = g.step0 + q.C < g.T ? g.step0 + q.C : g.T;
    g.step1 = run.own0 + q.W < g.T ? run.own0 + q.W : g.T;
    g.d0 = g.step1 == g.T ? start : nullptr;
    g.dout = q.fin + c * DP;
    run.warm = q.warm + c * DP;
    fused_draw_walk<DP, true>(g, run);
}
