// Dense engine, mid-sized states (16 < d <= 64, p <= 16), across the chip: the persistent passes of tgp_dense_fused.hpp cut into chunks of
// consecutive steps, one workgroup per chunk (the idea of the sweep engine, docs/DESIGN_HISTORY.md 3.14, which does not depend on d).
//
// The Kalman filter forgets its start state, so chunk c = [s_c, s_c+1) starts W steps early from the model's x0 and has (nearly) the sequential
// pass's state when it reaches s_c; the Bryson-Frazier adjoints forget likewise, so the backward chunk starts Wb steps late from
// (lambda, Lambda) = 0. Nothing is assumed about W: every chunk stores the state its warm-up reached at the crossing and the state its own run
// reached at its far end, and dk_chunk_close compares each warm-up state with the neighbour's run state -- the state the sequential pass
// would have handed over if the neighbour's own start was right, by induction from chunk 0 (which starts at step 0 and is exact). The host
// repeats a pass whose check fails with a longer warm-up, or runs the sequential passes (tgp_dense.hip: fused_filter, fused_posterior_marginals).
//
// The chunks are independent: no atomics, no waiting between workgroups; the stream orders the close kernel behind them. During a warm-up
// nothing is written -- outputs, records, log-likelihood terms of those steps belong to the neighbour.
//
// Included by tgp_dense.hip behind tgp_dense_fused.hpp (namespace tgp_dense).
#pragma once

struct ChunkGeom {
    int64_t C = 0;                     // steps per chunk (the last one may be shorter)
    int64_t W = 0;                     // warm-up steps (forward kernel: in front of the chunk; backward kernel: behind it)
    double* warm = nullptr;            // [chunks][DP DP + DP] state at the crossing from the warm-up into the chunk
    double* fin = nullptr;             // [chunks][DP DP + DP] state at the far end of the chunk's own run
    double* slots = nullptr;           // [chunks][4] forward: lml, missing count, first bad step + 1
};

// forward: chunk c owns [c C, min(T, (c + 1) C)) and starts at max(0, c C - W) from x0
template <int DP>
__global__ __launch_bounds__(256) void dk_chunk_filter(const FusedArgs g0, const ChunkGeom q) {
    constexpr int64_t NST = (int64_t)DP * DP + DP;
    const int64_t c = blockIdx.x;
    FusedArgs g = g0;
    FusedChunkRun run;
    run.own0 = c * q.C;
    g.step0 = run.own0 > q.W ? run.own0 - q.W : 0;
    g.step1 = run.own0 + q.C < g.T ? run.own0 + q.C : g.T;
    g.xfin = q.fin + c * NST;
    run.warm = q.warm + c * NST;
    run.slot = q.slots + c * 4;
    fused_filter_walk<DP, true>(g, run);
}

// backward: chunk c owns the same steps, walked downwards from min(T, (c + 1) C + W) with (lambda, Lambda) = 0 there; `fin` is the pair
// after the transition into step c C - 1 (what dk_fused_smooth carries between launches), the reference of chunk c - 1's warm-up
template <int DP>
__global__ __launch_bounds__(256) void dk_chunk_smooth(const FusedSmoothArgs g0, const ChunkGeom q) {
    constexpr int64_t NST = (int64_t)DP * DP + DP;
    const int64_t c = blockIdx.x;
    FusedSmoothArgs g = g0;
    FusedChunkRun run;
    g.step0 = c * q.C;
    run.own0 = g.step0 + q.C < g.T ? g.step0 + q.C : g.T;
    g.step1 = run.own0 + q.W < g.T ? run.own0 + q.W : g.T;
    g.first = 1;
    g.adj = q.fin + c * NST;
    run.warm = q.warm + c * NST;
    fused_smooth_walk<DP, true>(g, run);
}

// Closes a pass (one workgroup). Hand-over i = 0 .. npairs - 1 compares x[i] with its reference ref[i] (nst doubles each): the largest
// |x - ref| over the largest |ref| entry. out[0] = the worst of them, out[1] = status bits (1: a distance above tol, 4: a chunk met a
// non-positive innovation variance, 8: a non-finite state). With slots (the forward pass) and no bit 1 / 8, the chunks' terms are added to
// result8 in chunk order by one thread -- two calls give the same bits.
constexpr int kCloseThreads = 1024;
__global__ __launch_bounds__(kCloseThreads) void dk_chunk_close(const double* x, const double* ref, int nst, int npairs, const double* slots, int nchunks,
                                                               double tol, double* result8, double* out) {
    __shared__ double sdist[kCloseThreads / 64];
    __shared__ int sbadv[kCloseThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double worst = 0.0;
    int nonfinite = 0;
    for (int i = w; i < npairs; i += kCloseThreads / 64) {
        const double* xi = x + (int64_t)i * nst;
        const double* ri = ref + (int64_t)i * nst;
        double dmax = 0.0, rmax = 0.0;
        for (int e = lane; e < nst; e += 64) {
            const double a = xi[e], b = ri[e];
            if (!(fabs(a) <= 1e300) || !(fabs(b) <= 1e300)) nonfinite = 1;
            dmax = fmax(dmax, fabs(a - b));
            rmax = fmax(rmax, fabs(b));
        }
        for (int o = 32; o > 0; o >>= 1) {
            dmax = fmax(dmax, __shfl_xor(dmax, o));
            rmax = fmax(rmax, __shfl_xor(rmax, o));
        }
        worst = fmax(worst, dmax / fmax(rmax, 1e-300));
    }
    for (int o = 32; o > 0; o >>= 1) nonfinite |= __shfl_xor(nonfinite, o);
    if (lane == 0) {
        sdist[w] = worst;
        sbadv[w] = nonfinite;
    }
    __syncthreads();
    if (tid == 0) {
        double dist = 0.0;
        int status = 0;
        for (int k = 0; k < kCloseThreads / 64; ++k) {
            dist = fmax(dist, sdist[k]);
            if (sbadv[k]) status |= 8;
        }
        if (!(dist <= tol)) status |= 1;
        double lml = 0.0, nmiss = 0.0, bad = 0.0;
        if (slots) {
            for (int c = 0; c < nchunks; ++c) {
                lml += slots[4 * c];
                nmiss += slots[4 * c + 1];
                const double b = slots[4 * c + 2];
                if (b != 0.0 && (bad == 0.0 || b < bad)) bad = b;
            }
            if (!(fabs(lml) <= 1e300)) status |= 8;
            if (bad != 0.0) status |= 4;
            if (!(status & (1 | 8))) {
                result8[0] += lml;
                result8[1] += nmiss;
                if (bad != 0.0 && result8[2] == 0.0) result8[2] = bad;
            }
        }
        out[0] = dist;
        out[1] = (double)status;
    }
}
