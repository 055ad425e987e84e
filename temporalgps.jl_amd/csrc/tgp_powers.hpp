// The dense-power one-launch kernels: prior draws, _filter, the evaluated posterior, the adjoint gradient at d <= 6, and
// logpdf / posterior marginals / posterior draws of the models the modal plan declines -- each ONE kernel over the series behind a head the
// host runs, on dense powers of the transition (tgp_steady_plan.hpp builds them).  The kernels share their scan blocks (tgp_powers.hip, top).
#pragma once
#include <hip/hip_runtime.h>

#include "tgp_steady_plan.hpp"

namespace tgp_powers {

// Host plans of the filter / posterior / rand one-launch paths.  Defined in tgp_powers.hip only: its host code is built with -mavx2 -mfma like
// tgp_modal.hip's (one set of host compile flags for the plan header's inline functions), behind tgp_modal::host_cpu_ok -- a host without
// AVX2 gets a plan that declines.
void plan_filter(const tgp_plan::ModelHost& m, long long T, tgp_plan::FilterPlan& fp);
void plan_filter_head(const tgp_plan::ModelHost& m, const tgp_plan::FilterPlan& fp, const double* y, double* mout, double* Pout, double* mu_end, double* quad);
bool plan_posterior_head(const tgp_plan::ModelHost& m, const tgp_plan::FilterPlan& fp, const double* y, double* Gh, double* gh, double* Lh, double* Gss,
                         double* Lss, double* mu_end, double* quad);
void plan_rand(const tgp_plan::ModelHost& m, tgp_plan::RandPlan& rp);

// rand of an LTI model with the draws supplied (lgssm.jl:65-91; Forward, scalar observations, d <= tgp_plan::kRandMaxD): ONE kernel over the
// draws -- eps_t [T][d], eps_e [T] read once, y [T] written once -- by the same span / halo / in-tile-scan structure, on the dense powers
// of the open-loop transition (tgp_plan::build_rand).  x0: the drawn initial state (host).  Enqueues on `stream`; 0 or a hipError_t.
int rand_lti(hipStream_t stream, const tgp_plan::RandPlan& plan, const double* x0, const double* eps_t, const double* eps_e, long long T, double* y,
             const char** kname);
// steps a workgroup of k_rand_one owns (its tiles minus the run-in in front), and the workgroups of a T-step draw (no head: the first one starts at step 0)
long long rand_span(const tgp_plan::RandPlan& plan);
long long rand_workgroups(const tgp_plan::RandPlan& plan, long long T);

// _filter of an LTI model behind its head (tgp_plan::build_filter / filter_head; d <= tgp_plan::kRandMaxD): the steps [nhs, T) in ONE kernel --
// y read once, the filtered means [T][d] and covariances [T][d d] written once (either may be nullptr), sum r^2 per workgroup into `part`
// (pinned host memory, at least filter_workgroups() values).  mu_start: the predicted mean of step nhs (host).
// posterior(model, y) (lgssm.jl:193-221, :231-238) rides on it: behind the head the reverse-time transition G and its noise L are constants
// (Gss, Lss: d d doubles each, column-major, host) -- two more fills -- and g_(t+1) = m_t - G mu_(t+1) is at hand where m_t is; `fin` (pinned
// host memory, d doubles) receives the last filtered mean.  G, L [T][d d], g [T][d] (device); the steps [0, nhs) of G, L and [0, nhs] of g
// are the caller's (tgp_plan::posterior_head).
struct PosteriorOut {
    const double *Gss, *Lss;
    double *G, *g, *L, *fin;
};
long long filter_span(const tgp_plan::FilterPlan& plan);
long long filter_workgroups(const tgp_plan::FilterPlan& plan, long long T);
int filter_lti(hipStream_t stream, const tgp_plan::FilterPlan& plan, const double* mu_start, const double* y, long long T, double* m_out, double* P_out,
               double* part, const PosteriorOut* posterior = nullptr);

// The device half of d logpdf / d (model blocks) of an LTI model by ONE reverse-time pass behind the head, in ONE kernel (d <= 6):
// forwards mu' = Phi mu + a + (A K) u, backwards psi = Phi' psi + h r / S, and the sums SA = sum psi_{t+1} mu_t', Sa, Sk = sum psi_{t+1} r_t,
// Srm = sum r_t mu_t, Sr, sum r^2 over the steps [nhs, T) -- d^2 + 3 d + 2 values per workgroup into `part` (pinned host memory,
// adjoint_workgroups() x adjoint_sums(d) values), psi at step nhs into psi_out (pinned, d values).  tgp_adjoint::finish does the head and the rest.
constexpr int kAdjointMaxD = 6;
inline int adjoint_sums(int d) { return d * d + 3 * d + 2; }
long long adjoint_span(const tgp_plan::FilterPlan& plan);      // (a halo at both ends)
long long adjoint_workgroups(const tgp_plan::FilterPlan& plan, long long T);
// The head beside the kernel (as SmoothCall's): workgroup 0 copies the head's nhs observations to head_in (pinned) and raises head_in_flag; the
// host runs the head forwards and answers with the predicted mean of step nhs in mu0 (pinned) + mu0_flag; flags hold 2 seq.  mu_start is then unused.
struct HeadHandover {
    double* head_in = nullptr;
    long long* head_in_flag = nullptr;
    const double* mu0 = nullptr;
    const long long* mu0_flag = nullptr;
    long long seq = 0;
};
int adjoint_lti(hipStream_t stream, const tgp_plan::FilterPlan& plan, const double* mu_start, const double* y, long long T, double* part, double* psi_out,
                const HeadHandover* handover = nullptr);

// logpdf + posterior marginals of an LTI model behind its head in ONE kernel on DENSE powers of the closed loop (forwards) and of the settled
// reverse-time transition (backwards): the models the modal plan declines (d <= tgp_plan::kRandMaxD).  The head runs on the host
// (plan_smooth_head_*: forwards before the launch, its data-free tables beside the kernel, backwards behind it from xi_out).
// mean == nullptr: logpdf only.  part: smooth_workgroups() values, xi_out: d values, tvb: tgp_plan::kTailMax values -- pinned host memory.
struct SmoothCall {
    long long T = 0;
    const double *y = nullptr, *Rnew = nullptr;      // device
    int rnew_per_step = 0;
    const double* tvb = nullptr;
    double *mean = nullptr, *var = nullptr;          // device
    double *part = nullptr, *xi_out = nullptr;
    // The head beside the kernel (tgp_modal::overlap_allowed()): the launch does not wait for the head's forward recursion, and nothing between the launch
    // and the end of the kernel goes through a stream (a copy on a second stream may share the kernel's hardware queue and wait for it: measured --
    // the kernel would wait for the host, the host for the copy, the copy for the kernel).  Everything is handed over through pinned memory:
    //   head_in / head_in_flag   workgroup 0 copies the head's nhs observations (and, with rnew_per_step, its nhs new noise variances) there
    //                            first thing (nullptr: the caller's inputs are host arrays already);
    //   mu0 / mu0_flag           the host's answer: the predicted mean of step nhs (workgroup 0 waits for it, bounded);
    //   xi_out / xi_flag         raised by workgroup 0 once xi at step nhs is known: the host runs the head backwards;
    //   head_out / head_out_flag the head's nhs means and nhs variances from the host; a workgroup from the middle of the dispatch waits for them (bounded) and writes
    //                            them to mean / var [0, nhs).
    // Flags hold 2 seq once raised.  mu0_flag == nullptr: mu_start by value, head outputs are the caller's to write.
    double* head_in = nullptr;
    const double* mu0 = nullptr;
    const double* head_out = nullptr;
    long long *head_in_flag = nullptr, *xi_flag = nullptr;
    const long long *mu0_flag = nullptr, *head_out_flag = nullptr;
    long long seq = 0;
    // A DRAW from the posterior instead of its marginals (rand of the reverse-time model, lgssm.jl:65-91 / :193-221; d <= kSmoothRandMaxD):
    // eps_t [T][d], eps_e [T] (device), `mean` receives the draw, `var` stays unused; U (d d, row-major, upper): chol(L_settled + 1e-9 I).U,
    // v0 = G xi_T, s0 = h' xi_T with xi_T = chol(P_final + 1e-12 I).U' eps_0 (tgp_plan::smooth_rand_factors).  With the head beside the kernel,
    // head_in also receives the head's eta [nhs] and eps [nhs][d] behind y | Rnew (offsets 2 nhs, 3 nhs).
    // an emission offset per step (device, [T]; a mean function at the inputs: lti_sde.jl:118-131) instead of the plan's one value; the gains do not
    // see it.  With the head beside the kernel head_in receives the head's offsets at offset 10 nhs (the host's head functions take them as `hh_t`).
    const double* hh_t = nullptr;
    const double *eps_t = nullptr, *eps_e = nullptr;
    const double *U = nullptr, *v0 = nullptr;
    double s0 = 0.0;
};
constexpr int kSmoothRandMaxD = 6;
void plan_smooth(const tgp_plan::ModelHost& m, long long T, tgp_plan::SmoothPlan& sp, double* tvb, bool post = true);      // post = false: logpdf only (tvb unused)
void plan_smooth_head_forward(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp, const double* y, double* mu_end, double* quad, const double* hh_t = nullptr);
bool plan_smooth_head_tables(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp);
void plan_smooth_head_backward(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp, const double* y, const double* lam, double* mean, double* vb);
bool plan_smooth_rand_factors(const tgp_plan::SmoothPlan& sp, const double* eps0, double* U, double* v0, double* s0);      // (behind plan_smooth; false: not positive definite)
void plan_smooth_head_backward_rand(const tgp_plan::ModelHost& m, const tgp_plan::SmoothPlan& sp, const double* y, const double* delta, const double* eps_e,
                                    const double* eps_t, const double* rn, bool rn_per_step, double* out);
// steps a workgroup owns (its tiles minus the halo in front and -- with the backward half -- behind), and the workgroups of a T-step call
long long smooth_span(const tgp_plan::SmoothPlan& sp, bool post = true);
long long smooth_workgroups(const tgp_plan::SmoothPlan& sp, long long T, bool post = true);
int smooth_lti(hipStream_t stream, const tgp_plan::SmoothPlan& sp, const double* mu_start, const SmoothCall& c);

}  // namespace tgp_powers
