// Stationary-gain engine, STREAMING posterior kernel (round 6): logpdf + posterior marginals of an LTI model with one noise variance,
// scalar observations and no missing data behind its head -- what k_steady_one computes (tgp_modal.hip: lgssm.jl:99-238, lgc.jl:46-52,247-257 in the
// modal coordinates of the stationary closed loop), with the workgroups made persistent:
//   * 2048 waves, one RUN of consecutive 1024-step tiles each (64 lanes x 16 steps); a wave streams its run through ONE 8 KB slice of LDS, the next
//     tile's observations travelling while the current one is in work; the filter state passes from tile to tile exactly;
//   * per tile the zero-start sweeps + one DPP scan + the WJ / WG corrections of k_steady_one -- at sixteen steps per lane the scans cost half of what
//     they cost there per step, and nothing is chained through LDS or barriers;
//   * the backward recursion needs the NEXT tile's innovations: a tile's outputs are finished one tile late, from the left-edge state of the tile behind
//     it (tiles are longer than the halo: whatever lies further right has decayed by 2^-64); a run's last tile takes it from a `ghost` pass over the
//     first halo steps of the next run, a run's first tile its entry state from a state-only pass over the halo steps in front of it.
// The Modal handed to this unit is the input-normalised form of tgp_stream_form.hpp; z0p and zeta_out are in its coordinates (tgp_modal.hip maps them).
// Same host protocol as k_steady_one with the head on the host (tgp_modal.hip `complete`): head_in / z0p / zeta_out / head_out and their flags, the
// tail variances out of the pinned tables behind their stage flag, sum r^2 per workgroup into `part` -- as a (value, check) record behind the workgroup's
// last acknowledged output store: mean and var are stored write-through, and the host may end the call on the records.
#pragma once
#include <hip/hip_runtime.h>

#include "tgp_steady_plan.hpp"

namespace tgp_post {

constexpr int kNW = 8, kN = 16, kTile = 64 * kN, kMaxWG = 256;
constexpr int kMaxD = 8;

struct Geometry {
    long long G = 0, R = 0, C = 1;      // tiles behind the head, runs (one wave each), tiles per run in the middle of the series
    int nwg = 0;
};
// the path serves the call: a halo inside one tile
bool applies(const tgp_plan::Modal& md, long long T);
Geometry choose_geometry(const tgp_plan::Modal& md, long long T);

struct Call {
    long long T = 0;
    const double* y = nullptr;          // device
    const double* Rnew = nullptr;       // device: one value, or T values when rnew_per_step
    int rnew_per_step = 0;
    double *mean = nullptr, *var = nullptr;      // device
    // pinned host memory (the protocol of tgp_modal.hip's host head)
    const double* htab = nullptr;       // packed tables: [0] n1, tail variances at tvb_off (behind stage flag 2)
    int tvb_off = 0;
    const long long* flag = nullptr;    // the stages' flags
    double* part = nullptr;             // [nwg] (sum r^2, check) pairs, one per workgroup (check = the sum's bits ^ tgp_lml::record_key(seq))
    double* head_in = nullptr;
    const double* z0p = nullptr;
    double* zeta_out = nullptr;
    const double* head_out = nullptr;
    long long* hflag = nullptr;
    long long seq = 0;
    void* xch = nullptr;                // device memory, xch_bytes(): the runs' exchange records (zeroed once; sequence numbers only grow)
};
// the development stamps of TGP_POST_DBG=16 (two per run) sit behind the largest record table
constexpr size_t kStampOff = 2 * (size_t)kMaxWG;
constexpr size_t part_doubles() { return kStampOff + 2 * (size_t)kMaxWG * kNW; }
// May the host take the launch's end from the records?  Only if every output byte is written through and acknowledged in front of them: a noise variance
// per step keeps plain stores (its tiles go out element by element), and such a call ends on the stream's synchronisation as before.
inline bool records_end(const Call& c) { return !c.rnew_per_step; }
inline size_t xch_bytes() { return (size_t)kMaxWG * kNW * kMaxD * 16; }
int enqueue(hipStream_t stream, const tgp_plan::Modal& md, const Geometry& g, const Call& c, const char** kname);

}  // namespace tgp_post
