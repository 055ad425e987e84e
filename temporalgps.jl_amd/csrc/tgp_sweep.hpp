// The sweep engine (round 5): logpdf and posterior marginals of Forward models whose GAINS vary in time -- a missing-data mask,
// a noise variance per step, irregular spacing (transitions exp(F dt_k) in closed form) -- scalar observations, d <= 4.  What the
// reference's predict path produces (posterior_lti_sde.jl:20-37,97-131; missings.jl:25-41; lti_sde.jl:135-146) and what the stationary-gain
// engines (tgp_steady.hip, tgp_modal.hip) cannot serve: there the covariance half of the recursion is constant behind a head, here it
// depends on every step.
//
// One launch.  A lane owns a CHUNK of C consecutive steps and runs the reference's sequential recursion over it in registers (state
// (m, packed P): 9 doubles at d = 3 -- no scan elements, no carries between workgroups).  What a chunk needs from the steps before it is
// its start state, and the filter FORGETS: started from the stationary prior W steps early, it has the true state to rounding at the
// chunk's first step.  So every lane first warms up over the last W steps of its own chunk (the result is the NEXT lane's start state: one
// shift across the wave), then runs its chunk for real.  Backwards the same: the smoothing state at a chunk's end is the next lane's
// smoothing state at its first step, which that lane gets to rounding from a warm-up over its first Wb steps.  The filtering states a
// backward step needs are recomputed block by block from checkpoints (one state per B steps, written by the forward run) into LDS.
// A wave = 64 consecutive chunks, 62 of them its own (lane 0 only warms up for lane 1, lane 63 only for lane 62); waves are independent.
// Nothing is assumed about W: the run from the handed-over start must reproduce the warm-up's end state (and the same backwards) to
// `tol`, else the call reports it and the host repeats it with longer warm-ups (or hands it to the general engine).
//
// A draw from the posterior (k_sweep_draw) is the same forward half and, backwards, the reverse-time model's sample path instead of its
// marginals: a state of d doubles walks back over the chunk from the next lane's sample state of ITS first step, which that lane composed during its
// forward run over its first Wd steps from zero deviation (the walk forgets as the smoother does); the hand-over is checked on the sample states.
//
// The gradient of the log marginal likelihood (k_sweep_adjoint; LTI form) is the same forward half and, backwards, the adjoint of the
// recursion: (l, L) = d logpdf / d (m, P) of a filtering state, as large as the state, walks back over the chunk from the next lane's adjoint in front
// of ITS first step, which that lane got from a walk over its own first Wa steps from zero (the adjoint forgets at the filter's rate); the hand-over is
// checked on the adjoints.  A lane sums the gradients with respect to the shared blocks over its steps, the wave adds its lanes' sums, the host the waves'.
// SDE-described models (k_sweep_adjoint_sde): the same walk with the transitions built from the gaps; d logpdf / d A_t of a step is contracted
// on the spot into sums over the closed form's coefficients (lam, N1, N2) and the stationary covariance.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "tgp_sweep_plan.hpp"

namespace tgp_sweep {

constexpr int64_t kMinT = 2048;      // shorter series stay on the general engine (a chunk must hold the warm-up)

struct Engine;
Engine* create();
void destroy(Engine* e);

struct Call {
    int64_t T = 0;
    const double* y = nullptr;            // device
    const uint8_t* mask = nullptr;        // device or null
    const double* R = nullptr;            // device per-step noise variance, or null (shared)
    const double* hh = nullptr;           // device per-step emission offset, or null (shared)
    const double* tau = nullptr;          // device [T] gaps (SDE)
    const double* Rnew = nullptr;         // device
    int rnew_per_step = 0;
    double* mean = nullptr;               // device; null: logpdf only
    double* var = nullptr;
    // a posterior draw instead (y_out set; mean / var null): k_sweep_draw, k_sweep_group_draw (5 <= d <= 8)
    const double* eps_t = nullptr;        // device [T][d]: row t drives the reverse-time transition out of step t (row 0 unused)
    const double* eps_e = nullptr;        // device [T]
    double eps_0[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};      // the start x_(T-1), d entries: travels in the kernel arguments
    double* y_out = nullptr;              // device [T]
    // the adjoint gradient instead (mean / var / y_out null): k_sweep_adjoint (LTI form), k_sweep_adjoint_sde (SDE form)
    bool adjoint = false;
    double* gh_steps = nullptr;           // device [T] or null: d logpdf / d h_t, d logpdf / d R_t of every step (zero at missing ones)
    double* gR_steps = nullptr;
};
// where adjoint_blocks writes the gradient with respect to the shared blocks (host, column-major, any null; ghh / gR: the sums over the observed steps)
struct AdjointOut {
    double *gA = nullptr, *ga = nullptr, *gQ = nullptr, *gH = nullptr, *ghh = nullptr, *gR = nullptr, *gx0m = nullptr, *gx0P = nullptr;
};

// the same for an SDE-described model (host, column-major, none null): the sums over the closed form's coefficients (lam per row, N1, N2 = N^2 / 2), the
// stationary covariance (symmetric), the explicit first transition; the caller finishes d logpdf / d F by the transpose of its own coefficient map
struct AdjointSdeOut {
    double *gl = nullptr, *gN1 = nullptr, *gN2 = nullptr, *gPinf = nullptr, *gA1 = nullptr, *ga = nullptr, *gH = nullptr, *ghh = nullptr, *gR = nullptr,
           *gx0m = nullptr, *gx0P = nullptr;
};

// The gradient with respect to the shared blocks from the waves' records of an adjoint call (pinned host memory, `stride` doubles per wave: 4 status words,
// then gA d*d | ga d | gQ packed | gH d | sum gh_t | sum gR_t | gx0m d | gx0P packed): added in wave order -- two calls on the same series give the same
// bits -- and the packed blocks unpacked to full symmetric ones.  Both sweep engines leave this record (tgp_sweep.hip, tgp_sweep_group.hip).
inline void adjoint_blocks_from_parts(const double* part, int64_t nwaves, int stride, int d, const AdjointOut& o) {
    const int dd = d * d, ds = d * (d + 1) / 2, ng = stride - 4;
    double g[group_adjoint_sums(kGroupMaxD)] = {0.0};      // (the largest record: d = 8)
    for (int64_t i = 0; i < nwaves; ++i) {
        const double* q = part + (size_t)i * stride + 4;
        for (int k = 0; k < ng; ++k) g[k] += q[k];
    }
    const double *gA = g, *ga = gA + dd, *gQ = ga + d, *gH = gQ + ds, *gs = gH + d, *gm = gs + 2, *gP = gm + d;
    auto unpack = [d](const double* packed, double* full) {
        for (int j = 0; j < d; ++j)
            for (int i = 0; i < d; ++i) full[i + j * d] = packed[pidx(i, j)];
    };
    if (o.gA) std::memcpy(o.gA, gA, sizeof(double) * dd);
    if (o.ga) std::memcpy(o.ga, ga, sizeof(double) * d);
    if (o.gQ) unpack(gQ, o.gQ);
    if (o.gH) std::memcpy(o.gH, gH, sizeof(double) * d);
    if (o.ghh) *o.ghh = gs[0];
    if (o.gR) *o.gR = gs[1];
    if (o.gx0m) std::memcpy(o.gx0m, gm, sizeof(double) * d);
    if (o.gx0P) unpack(gP, o.gx0P);
}

// Chooses the geometry (chunk length, warm-ups) for this model and series; false: the engine declines (`why` says so).
// w_hint / wb_hint: warm-ups a previous call on the same bound model needed (0: estimate from the model).
// wd_hint: the draw's warm-up (0: the backward warm-up's value; a draw call that passes one may lengthen the chunk to hold it).
// wa_hint: the adjoint's warm-up (0: the forward warm-up's value; likewise).
bool plan(Engine* e, const ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, std::string* why, int wd_hint = 0, int wa_hint = 0);
int enqueue(Engine* e, hipStream_t stream, const Call& c, const char** kernel_name, std::string* err);
const char* kernel_name(int d, bool sde, bool post, bool draw = false);
const char* adjoint_kernel_name();
const char* adjoint_sde_kernel_name();
// After the stream has been synchronised.  status bits: 1 forward warm-up too short, 2 backward warm-up too short, 4 not positive definite,
// 8 non-finite values.  *w / *wb: the warm-ups the call ran with.  A draw: bit 2 and *dist_b are the draw warm-up's (*wd), the returned value is 0.
// An adjoint call: bit 2 and *dist_b are the adjoint warm-up's (*wa), the returned value is the log marginal likelihood.
double finish(Engine* e, int* status, int* w, int* wb, double* dist_f, double* dist_b, int* wd = nullptr, int* wa = nullptr);
// Behind finish of an adjoint call whose status is clean: the waves' sums, added in wave order.
void adjoint_blocks(const Engine* e, const AdjointOut& out);
void adjoint_blocks_sde(const Engine* e, const AdjointSdeOut& out);
// geometry of the last plan (diagnostics / tests)
void geometry(const Engine* e, int* C, int* W, int* Wb, int64_t* nwaves, int* Wd = nullptr);
// test hook: force the geometry of the next plan (0: automatic)
void force_geometry(Engine* e, int C, int W, int Wb, int Wd = 0, int Wa = 0);

}  // namespace tgp_sweep
