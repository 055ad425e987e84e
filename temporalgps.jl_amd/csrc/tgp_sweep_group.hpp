// The group sweep: the sweep engine's algorithm (tgp_sweep.hpp) for state dimensions 5 .. 8 -- logpdf and posterior marginals of
// Forward models in LTI form (shared A, a, Q, H; scalar observations) whose gains vary in time: a missing-data mask, a noise variance per step,
// an emission offset per step.  At these d a lane cannot hold the state (m, packed P) of a chunk in registers (tgp_sweep_plan.hpp kMaxD), so a
// chunk of C steps belongs to a GROUP of 8 lanes, lane j holding column j of every matrix as in tgp_group.hpp: ~10 d doubles per lane.
//
// One launch, one wave per workgroup, a wave = 8 groups = 8 consecutive chunks.  Forwards every group warms up over the last W steps of its own
// chunk from the stationary prior -- the result is the NEXT group's start state, one shift by 8 lanes -- and then runs its chunk for real: the
// sums of the log marginal likelihood over its observed steps, a checkpoint of the state every B steps (posterior calls).  Backwards (posterior
// calls) the RTS step in the reference's gain form with its 1e-10 jitter: a group continues from the next group's smoothing state of ITS first
// step, which that group gets from a backward run over its own first Wb steps; the filtering states a backward step needs are recomputed block
// by block from the checkpoints into LDS.  Both hand-overs are checked to `tol` as in the lane sweep and the host repairs or declines the same way.
// Group 0 of a wave only warms up for group 1, and in a posterior call group 7 only warms up (backwards) for group 6: waves are independent, 7 of 8
// groups own output in a logpdf call, 6 of 8 in a posterior call.
//
// The gradient of the log marginal likelihood (k_sweep_group_adjoint) is the posterior call's geometry and forward half and, backwards, the
// adjoint of the recursion (tgp_sweep.hpp) in the column layout: lane j holds l_j and column j of L; a group continues from the next group's
// adjoint in front of ITS first step, which that group gets from a walk over its own first Wa steps from zero; the hand-over is checked on the adjoints.
// A lane sums column j of the block gradients over its group's steps, the wave adds its six owned groups, the host the waves.
//
// A draw from the posterior (k_sweep_group_draw) is the same geometry and forward half and, backwards, the reverse-time model's sample path
// (tgp_sweep.hpp) instead of its moments: the sample state is one double per lane; a group continues from the next group's sample of ITS first
// step, which that group gets from a walk over its own first Wd steps from the filtering mean with the real draws; the hand-over is checked on the samples.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "tgp_sweep.hpp"

namespace tgp_sweep_group {

struct Engine;
Engine* create();
void destroy(Engine* e);

// The geometry for this model and series (tgp_sweep_plan.hpp plan_group); false: the engine declines (`why` says so).  post: the call asks for the
// posterior marginals.
// adjoint: the call asks for the gradient (k_sweep_group_adjoint) -- the posterior call's geometry with the adjoint's warm-up Wa in the backward
// slot: wb_hint is a Wa that a previous call needed (0: the forward warm-up's value), and a forced Wb forces Wa.
// draw: the call asks for a draw from the posterior (k_sweep_group_draw) -- the same with the draw's warm-up Wd in the backward slot: wb_hint
// is a Wd that a previous call needed (0: the backward warm-up's estimate).
bool plan(Engine* e, const tgp_sweep::ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, bool post, std::string* why, bool adjoint = false,
          bool draw = false);
// c: the lane sweep's call record; y, mask, R, hh, Rnew, mean, var are read (mean == null: logpdf only); c.adjoint: the gradient instead (gh_steps,
// gR_steps: device [T] or null), on an adjoint plan; c.y_out set: a draw instead (Rnew, eps_t, eps_e, eps_0), on a draw plan
int enqueue(Engine* e, hipStream_t stream, const tgp_sweep::Call& c, const char** kernel_name, std::string* err);
const char* kernel_name(bool post, bool sde = false);      // sde: the model is SDE-described (k_sweep_group_sde)
const char* adjoint_kernel_name();
const char* draw_kernel_name();
// After the stream has been synchronised: tgp_sweep::finish's status bits, warm-ups and distances.  An adjoint call: bit 2, *wb and *dist_b are the
// adjoint warm-up's; a draw call: the draw warm-up's, and the returned value is 0.
double finish(Engine* e, int* status, int* w, int* wb, double* dist_f, double* dist_b);
// Behind finish of an adjoint call whose status is clean: the waves' sums, added in wave order (gQ and gx0P symmetric).
void adjoint_blocks(const Engine* e, const tgp_sweep::AdjointOut& out);
void geometry(const Engine* e, int* C, int* W, int* Wb, int64_t* nwaves);
// test hook: force the geometry of the next plan (0: automatic)
void force_geometry(Engine* e, int C, int W, int Wb);

}  // namespace tgp_sweep_group
