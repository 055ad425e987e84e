// The tile sweep: the sweep engines' algorithm (tgp_sweep.hpp) for state dimensions 9 .. 16 -- logpdf and posterior marginals of Forward
// models in LTI form (shared A, a, Q, H; scalar observations) whose gains vary in time: a missing-data mask, a noise variance per step, an emission
// offset per step.  At these d a covariance is exactly ONE tile of v_mfma_f64_16x16x4_f64: the state is zero-padded to 16, d is a run-time argument and
// one instantiation set (XS = 0 .. 3, logpdf / posterior) serves every d.
//
// One launch, one wave per workgroup, a wave = one chunk of C consecutive steps.  P lives in the MFMA accumulator layout (lane (lr, lq), register r:
// row lq + 4 r, column lr), and A in registers as the four A-operands A[lr][lq + 4 r]: register r of P IS the B-operand of MFMA r, so A P costs four
// MFMAs and no data movement; P- = A (A P)' + Q four more, with Q as the accumulator's initial value, behind one transpose of A P through a padded
// LDS tile.  The scalar update runs in plain fp64 on the accumulator registers: P- H' by DPP sums inside the 16-lane rows and by sums across the four
// row groups, the rank-one downdate four FMAs per lane; m sits one component per lane.
//
// Forwards a wave warms up over the W steps in front of its chunk from the stationary prior, runs its chunk (log s and v^2 / s of its observed steps)
// and, for the check, repeats the warm-up its neighbour starts from -- the last W steps of its own chunk -- and compares it with its own run's end
// state (kTol).  Waves never wait for each other.  Posterior calls keep no covariance per step: the forward run leaves a record of 16 + 4 doubles per
// step (w = P- H', H P- H', H m-, v, s) and the backward run is the Bryson-Frazier recursion on (r, N), N a second accumulator-layout tile:
// N <- A' N A by the same eight MFMAs and one transpose, the observed step's (I - K H)' N (I - K H) + H' H / s as rank-one corrections;
// mean_t = H m- + w' r + h_t, var_t = H P- H' - w' N w + Rnew_t.  The (r, N) behind a chunk's last step come from a backward run over the Wb steps
// behind it from zero, on records the wave filters itself beyond its chunk; the check is the same run over the chunk's own first Wb steps against the
// chunk's own result (kTolBack).
//
// The gradient of the log marginal likelihood (k_sweep_tile_adjoint) is the same forward half with a checkpoint (m, P) every 8 steps in place
// of the record and, backwards, the adjoint of the recursion: (l, L) = d logpdf / d (m, P), L a second accumulator-layout tile.  A block's
// states are recomputed from its checkpoint into LDS; a step rebuilds A P and P- (eight MFMAs), takes its scalars from DPP sums, adds
// gA += mb m' + 2 Pb (A P) by four MFMAs whose operands are the registers Pb and A P already sit in, and hands back L <- A' Pb A by the backward
// sandwich.  The adjoint behind a chunk comes from a walk over the Wa steps behind it from zero; the check is the same walk over the chunk's own first Wa
// steps against the chunk's own result (kTolBack).  Every wave leaves one record of its sums; k_sweep_tile_adjoint_sum adds them in wave order.
//
// A draw from the posterior (k_sweep_tile_draw) is the same forward half with the same checkpoints and, backwards, the reverse-time model's
// sample path on supplied draws: x_(t-1) = m_f + G (x_t - m-) + chol(L + 1e-9 I).U' eps_t.  A step rebuilds A P and P- (eight MFMAs), factorises
// P- + 1e-10 I on the accumulator registers a pivot at a time and forward-substitutes [A P | x_t - m-] into [Z | q] in the same sweep, so that
// G (x_t - m-) = Z' q and L = P - Z' Z (four MFMAs on the registers Z sits in) need no back-substitution and no G; a second factorisation gives the noise.
// The x behind a chunk comes from a walk over the Wd steps behind it from x = m_f on the real draws; the check is the same walk over the chunk's own
// first Wd steps against the chunk's own x (kTolBack).  Nothing of size T x d^2 but the checkpoints.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "tgp_sweep.hpp"

namespace tgp_sweep_tile {

struct Engine;
Engine* create();
void destroy(Engine* e);

// The geometry for this model and series (tgp_sweep_plan.hpp plan_tile); false: the engine declines (`why` says so).  post: the call asks for the
// posterior marginals.  w_hint / wb_hint: warm-ups a previous call on the bound model needed (0: estimate).  An adjoint call plans with post = true and
// its warm-up Wa in the backward slot (0: the backward warm-up's estimate); a draw the same with its warm-up Wd.
bool plan(Engine* e, const tgp_sweep::ModelHost& m, int64_t T, int w_hint, int wb_hint, int num_cu, bool post, std::string* why);
// c: the lane sweep's call record; y, mask, R, hh, Rnew, mean, var are read (mean == null: logpdf only); c.adjoint: gh_steps, gR_steps instead of mean, var;
// c.y_out set: a draw instead (Rnew, eps_t, eps_e, eps_0)
int enqueue(Engine* e, hipStream_t stream, const tgp_sweep::Call& c, const char** kernel_name, std::string* err);
const char* kernel_name(bool post);
const char* adjoint_kernel_name();
const char* draw_kernel_name();
// Behind finish of an adjoint call whose status is clean: the gradient with respect to the shared blocks (Q and x0P symmetrised).
void adjoint_blocks(const Engine* e, const tgp_sweep::AdjointOut& out);
// After the stream has been synchronised: tgp_sweep::finish's status bits, warm-ups and distances.
double finish(Engine* e, int* status, int* w, int* wb, double* dist_f, double* dist_b);
void geometry(const Engine* e, int* C, int* W, int* Wb, int64_t* nwaves);
// test hook: force the geometry of the next plan (0: automatic)
void force_geometry(Engine* e, int C, int W, int Wb);

}  // namespace tgp_sweep_tile
