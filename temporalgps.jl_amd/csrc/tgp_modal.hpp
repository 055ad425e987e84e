// Stationary-gain engine, ONE-LAUNCH path (round 4): logpdf and posterior marginals of an LTI model with one noise variance,
// scalar observations and no missing data -- the reference's `Fill` layout for RegularSpacing inputs (src/gp/lti_sde.jl:148-160) -- as
//     host plan (tgp_steady_plan.hpp: covariance recursion to its fixed point, gains, variance tables, modal form; a few microseconds)
//   + ONE kernel over y (k_steady_one: reads y once, writes mean and var once; no pass before it, no carry kernel, no reduction kernel)
//   + the host's sum of the workgroups' partial sums of squares (they land in pinned host memory; the call synchronises anyway).
// It computes what tgp_steady.hip computes (same re-association of lgssm.jl:99-238, lgc.jl:46-52,247-257), in the modal coordinates of
// the stationary closed loop.  Applies when the plan says so (tgp_plan::Info::why == kOk); every other case stays on tgp_steady.hip /
// the general engine.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "tgp_steady_plan.hpp"

namespace tgp_modal {

struct Call {
    long long T = 0;
    const double* y = nullptr;      // device
    const double* Rnew = nullptr;   // device: one value, or T values when rnew_per_step
    int rnew_per_step = 0;
    double *mean = nullptr, *var = nullptr;      // device; nullptr: logpdf only
    // A time segment of the series (one rank of several): y, Rnew (per step), mean, var hold the steps [seg_lo, seg_hi) only; yl / yr the
    // `halo` observations in front of / behind them (device; unused at the series' ends).  Default: the whole series.
    long long seg_lo = 0, seg_hi = -1;
    const double *yl = nullptr, *yr = nullptr;
};

struct Engine;
Engine* create();
void destroy(Engine*);
// Host half: builds the plan of a T-step call of the model (nothing is kept from earlier calls).  false: the path does not apply (last_plan().why).
// logpdf_only: the call will be a logpdf over the whole series (no outputs, no segment) -- served by the streaming kernel of tgp_lml.hip.
bool plan(Engine*, const tgp_plan::ModelHost&, long long T, bool logpdf_only = false);
// TGP_OPT_STREAM_MIN_T: -1 the measured crossovers, 0 always, else the series length from which the streaming kernels serve
void set_stream_min_T(Engine*, long long min_T);
// the host's wait for a logpdf-only call's kernel: true once its last workgroup has said so through pinned memory (false: use the stream)
bool await_done(Engine*);
// TGP_STEADY_DEBUG, the last streaming call: the host's clock (steady_clock, ns) at its first sight of a head observation, of a record, of the last record
void debug_stamps(const Engine*, long long ns[3]);
// Enqueues the kernel of the planned call on `stream` (no synchronisation); *kname names it for the profile.
int enqueue(Engine*, hipStream_t stream, const Call&, const char** kname, std::string* err);
// Right behind enqueue: the tables half of the plan when plan() left it for now (the kernel's head wave and last tiles wait for it).
// false: that half declined -- synchronise, discard the outputs, run the call elsewhere.
bool complete(Engine*, long long T);
// Leaving between enqueue and complete (an error path): raise the flags the kernel may be waiting for, with the failure bit.  Harmless otherwise.
void abandon(Engine*);
// Once the stream has passed the kernel: the log marginal likelihood (a call over the whole series) ...
double finish(const Engine*, long long T);
// ... or the launch's share of the quadratic form (a segment): lml = -(T log 2pi + LS + (T - n0) logS + sum head_quad + iS sum ssq) / 2
void finish_parts(const Engine*, double* ssq, double* head_quad);
// the whole plan (both halves) without an engine: the pure host function tgp_steady_plan of the ABI
tgp_plan::Info plan_only(const tgp_plan::ModelHost&, long long T, tgp_plan::Modal&, tgp_plan::HeadTables&);
const tgp_plan::Info& last_plan(const Engine*);
const tgp_plan::Modal& last_modal(const Engine*);
// the kernel variant plan() chose for the call (profile label)
const char* kernel_name(const Engine*, bool posterior);
const char* kernel_name(const Engine*, const Call&);      // ... for this very call (pointer alignment and segment bounds are part of the choice)
void choose_geometry(int d, int halo, int* waves, int* steps_per_lane);

// false when the process runs with synchronous launches (HIP_LAUNCH_BLOCKING, AMD_SERIALIZE_KERNEL, ...) or TGP_MODAL_OVERLAP=0: a kernel
// that waits for a flag the host raises behind the launch would wait for itself
bool overlap_allowed();
// the host's wait for a flag in pinned memory the kernel on `stream` raises (value >= v): returns false once the stream has drained without it
bool await_host_flag(const long long* flag, long long v, hipStream_t stream);
// the host has AVX2 + FMA: the objects that instantiate the plan header's host functions (tgp_modal.o, tgp_powers.o) are built for them, and
// every plan entry declines without them
bool host_cpu_ok();

}  // namespace tgp_modal
