// Part of tgp_api.hip (included there, one translation unit): how a call reaches the stationary-gain scan engine (tgp_steady.hip), the one-launch form (tgp_modal.hip) and the sweep engine (tgp_sweep.hip).
// ---- stationary-gain scan engine (tgp_steady.hip) ------------------------------------------------------------------------------------
bool steady2_eligible(const tgp_handle* h, const uint8_t* missing, uint32_t flags) {
    // (an explicit TGP_OPT_CHUNK asks for the chunked-scan engine: the chunk length means nothing here)
    return h->opt_steady2 && h->steady2_state >= 0 && !h->is_dense && !h->sde && h->lti && h->p == 1 && h->mv.sR == 0 && h->ordering == 0 &&
           missing == nullptr && !(flags & TGP_REUSE_REDUCE) && tgp_steady::supports(h->d) && h->mv.T == h->T && h->opt_chunk == 0;
}
void steady2_begin(void* ctx, const char* name) {
    tgp_handle* h = static_cast<tgp_handle*>(ctx);
    h->steady2_scope = new LaunchScope(h, name);
}
void steady2_end(void* ctx) {
    tgp_handle* h = static_cast<tgp_handle*>(ctx);
    delete static_cast<LaunchScope*>(h->steady2_scope);
    h->steady2_scope = nullptr;
}
// Enqueues the call on the engine (y already staged in h->mv.y). mean_dev == nullptr: logpdf only.
int steady2_enqueue(tgp_handle* h, const double* Rnew_dev, bool rnew_per_step, double* mean_dev, double* var_dev, bool grad = false,
                    const tgp_steady::ShardDev* shard = nullptr, int phase = 0) {
    if (!h->steady2) h->steady2 = tgp_steady::create();
    tgp_steady::ModelDev md;
    md.d = h->d;
    md.A = h->mv.A; md.a = h->mv.a; md.Q = h->mv.Q; md.H = h->mv.H; md.hh = h->mv.h; md.R = h->mv.R;
    md.x0 = h->bx0.d();
    tgp_steady::CallDev cd;
    cd.T = h->T;
    cd.y = h->mv.y;
    cd.Rnew = Rnew_dev;
    cd.rnew_per_step = rnew_per_step ? 1 : 0;
    cd.mean = mean_dev;
    cd.var = var_dev;
    cd.result = h->result.d();
    cd.grad = grad;
    tgp_steady::Hooks hk;
    if (h->profile) {
        hk.ctx = h;
        hk.begin = steady2_begin;
        hk.end = steady2_end;
    }
    std::string err;
    if (shard) {
        if (tgp_steady::enqueue_shard(h->steady2, h->stream, md, cd, *shard, phase, hk, &err) != 0) return h->fail(TGP_EHIP, err);
        return TGP_OK;
    }
    if (tgp_steady::enqueue(h->steady2, h->stream, md, cd, hk, &err) != 0) return h->fail(TGP_EHIP, err);
    return TGP_OK;
}
// After CallTimer::finish: did the engine serve the call? (host_result[6]; 2 = it found on the device that it does not apply)
// ---- the one-launch form (tgp_modal.hip). Returns TGP_OK with *served = true when it ran the call (lml in *lml_out, outputs written);
// *served = false: it does not apply to this model / series -- nothing was enqueued.
// Behind a successful tgp_modal::enqueue with a deferred tables half the kernel waits for flags in pinned memory that only complete() raises:
// an exit in between (today there is none; any future one) must raise them with the failure bit.
struct ModalFlagGuard {
    tgp_modal::Engine* e;
    ~ModalFlagGuard() { tgp_modal::abandon(e); }
};
int modal_call(tgp_handle* h, const double* y, uint32_t flags, const double* Rnew, double* mean_out, double* var_out, double* lml_out, bool* served) {
    *served = false;
    if (!h->opt_modal || h->modal_state < 0 || h->hostm.empty()) return TGP_OK;
    if (!h->modal) h->modal = tgp_modal::create();
    static const bool dbg = getenv("TGP_STEADY_DEBUG") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    const int d = h->d;
    const size_t dd = (size_t)d * d;
    const double* q = h->hostm.data();
    tgp_plan::ModelHost mh;
    mh.d = d;
    mh.A = q; mh.a = q + dd; mh.Q = q + dd + d; mh.H = q + 2 * dd + d; mh.hh = q + 2 * dd + 2 * d; mh.R = h->has_R_over ? &h->R_over : q + 2 * dd + 2 * d + 1;
    mh.x0m = h->x0m.data();
    mh.x0P = h->x0P.data();
    tgp_modal::set_stream_min_T(h->modal, h->opt_stream_min_T);
    if (!tgp_modal::plan(h->modal, mh, h->T, /*logpdf_only=*/mean_out == nullptr && var_out == nullptr)) {
        h->modal_state = -1;
        if (getenv("TGP_STEADY_DEBUG") != nullptr) {
            const tgp_plan::Info& in = tgp_modal::last_plan(h->modal);
            fprintf(stderr, "[tgp modal] does not apply: why %d, n0 %d n1 %d halo %d cond %.3g / %.3g rho %.6f resid %.3g\n", in.why, in.n0, in.n1, in.halo, in.cond_f, in.cond_g, in.rho, in.resid);
        }
        return TGP_OK;
    }
    const auto tp1 = std::chrono::steady_clock::now();
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0;
    const bool rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    CallTimer tm(h, /*clear=*/false);
    const void* pR = nullptr;
    if (mean_out) TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    double *dm = nullptr, *dv = nullptr;
    TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
    TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
    tgp_modal::Call c;
    c.T = h->T;
    c.y = h->mv.y;
    c.Rnew = static_cast<const double*>(pR);
    c.rnew_per_step = (mean_out && !rshared) ? 1 : 0;
    c.mean = dm;
    c.var = dv;
    {
        std::string err;
        const char* kname = tgp_modal::kernel_name(h->modal, c);
        LaunchScope ls(h, kname);
        if (tgp_modal::enqueue(h->modal, h->stream, c, &kname, &err) != 0) return h->fail(TGP_EHIP, err);
    }
    const auto tp2 = std::chrono::steady_clock::now();
    ModalFlagGuard flag_guard{h->modal};      // (whatever path leaves this function from here on: the kernel is never left waiting for its tables)
    const bool tables_ok = tgp_modal::complete(h->modal, h->T);      // (the tables half of the plan, beside the kernel)
    const auto tp3 = std::chrono::steady_clock::now();
    tm.kernels_done();
    TRY(copy_back(h, mean_out, dm, nT, odev));
    TRY(copy_back(h, var_out, dv, nT, odev));
    if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
    // (a call on a streaming kernel ends on the workgroups' records in pinned memory: a logpdf-only call has nothing else to wait for, a posterior call's
    //  outputs are in device memory in front of its records -- unless they go back to the host behind the kernel, or the call is timed or profiled)
    const bool by_records = !h->timing && !h->profile && ((mean_out == nullptr && var_out == nullptr) || odev) && tgp_modal::await_done(h->modal);
    if (!by_records) HIPCHK(hipStreamSynchronize(h->stream));
    if (dbg) {
        const auto tp4 = std::chrono::steady_clock::now();
        auto us = [](auto a, auto b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
        fprintf(stderr, "[tgp modal host] plan core %.1f us, staging + launch %.1f, tables + copies %.1f, wait %.1f\n", us(tp0, tp1), us(tp1, tp2), us(tp2, tp3), us(tp3, tp4));
        if (by_records) {      // a streaming call that ended on its records: where its time went behind the launch's return, on the same clock
            long long ns[3];
            tgp_modal::debug_stamps(h->modal, ns);
            const long long t2 = std::chrono::duration_cast<std::chrono::nanoseconds>(tp2.time_since_epoch()).count();
            auto since = [&](long long t) { return t ? (double)(t - t2) * 1e-3 : -1.0; };
            fprintf(stderr, "[tgp modal host] us behind the launch's return: head observation seen %.1f, first record seen %.1f, last record seen %.1f\n", since(ns[0]), since(ns[1]),
                    since(ns[2]));
        }
    }
    read_timing(h);
    resolve_profile(h);
    if (!tables_ok) {      // declined behind the launch (a head step not positive definite, a smoother transient beyond the table): the older engines serve the call
        h->modal_state = -1;
        return TGP_OK;
    }
    const double lml = tgp_modal::finish(h->modal, h->T);
    note_served(h, Served::modal, tgp_modal::last_plan(h->modal).n0, lml, lml_out);
    h->modal_state = 1;
    *served = true;
    return TGP_OK;
}

// An explicit TGP_OPT_CHUNK or TGP_OPT_VARIANT asks for the chunked-scan engine's kernels (tests and A/B runs compare them with the one-launch
// paths): every one-launch fast path steps aside, as steady2_eligible always did (round-4 advice).
bool chunk_engine_requested(const tgp_handle* h) { return h->opt_chunk != 0 || h->variant_opt != 0; }

// ---- the sweep engine (tgp_sweep.hip, DESIGN 3.14): time-varying gains -------------------------------------------------------------------
// Forward models with scalar observations, d <= 4, whose transitions are one shared block (A, a, Q) or closed-form SDE transitions from the
// time stamps, H shared; the noise variance and the emission offset may be per step, steps may be missing.  The stationary-gain engines
// take what they can serve first (every block shared, one noise variance, nothing missing).
bool sweep_eligible(const tgp_handle* h, uint32_t flags) {
    if (!h->opt_sweep || h->sweep_state < 0 || h->is_dense || h->p != 1 || h->ordering != 0 || h->d > tgp_sweep::kMaxD) return false;
    // (explicit requests for the chunked-scan engine: a chunk length, a kernel variant, TGP_OPT_STEADY = 0 / 1, hipGraph replay of its launch chain)
    if ((flags & TGP_REUSE_REDUCE) || h->opt_chunk != 0 || h->variant_opt != 0 || !h->opt_steady2 || h->opt_graph != 0) return false;
    if (h->T < tgp_sweep::kMinT || h->mv.T != h->T || h->mv.sH != 0 || h->sweepm.empty()) return false;
    if (h->sde) return h->sde_closed && h->opt_sde_closed && !h->sde_coef_host.empty() && h->mv.sa == 0;
    return h->mv.sA == 0 && h->mv.sa == 0 && h->mv.sQ == 0;
}
// The group sweep (tgp_sweep_group.hip, DESIGN 4.10): the same conditions at 5 <= d <= 8, LTI form only (an SDE-described model's transition differs
// per chunk and cannot be the wave-wide broadcast the group kernels read).  Both engines share sweep_state, the forced geometry and tgp_sweep_info.
// Default routing (TGP_OPT_SWEEP = 1) takes only the (d, call) pairs whose median beat the general engine's at T = 1e6 AND 1e7
// (profiles/sweep_group_time.txt): logpdf at d = 6, 7, 8.  logpdf at d = 5 loses at 1e7 and the posterior kernel loses at every d at one length at
// least: those run here under TGP_OPT_SWEEP = 2 only (tests, A/B timing).
bool sweep_group_default_route(int d, bool post) { return !post && d >= 6; }
// explicit_call: an entry point of the engine's own (tgp_logpdf_adjoint_group), which the default routing does not filter.
bool sweep_group_eligible(const tgp_handle* h, uint32_t flags, bool post, bool explicit_call = false) {
    if (!h->opt_sweep || h->sweep_state < 0 || h->is_dense || h->p != 1 || h->ordering != 0 || h->sde) return false;
    if (h->d < tgp_sweep::kGroupMinD || h->d > tgp_sweep::kGroupMaxD) return false;
    if (!explicit_call && h->opt_sweep < 2 && !sweep_group_default_route(h->d, post)) return false;
    if ((flags & TGP_REUSE_REDUCE) || h->opt_chunk != 0 || h->variant_opt != 0 || !h->opt_steady2 || h->opt_graph != 0) return false;
    if (h->T < tgp_sweep::kGroupMinT || h->mv.T != h->T || h->mv.sH != 0 || h->sweepm.empty()) return false;
    return h->mv.sA == 0 && h->mv.sa == 0 && h->mv.sQ == 0;
}
// An SDE-described model at 5 <= d <= 8 (k_sweep_group_sde, DESIGN 4.13): sweep_eligible's SDE conditions (the closed form found and allowed, a and H
// shared) with sweep_group_eligible's others.  tgp_logpdf and tgp_[logpdf_and_]posterior_marginals (the draw and the gradient have
// explicit entries of their own, below), and under TGP_OPT_SWEEP = 2 only: no (d, call) pair is routed here by default (profiles/sweep_group_sde_time.txt has the measured medians
// beside the general engine's: a routing change would rest on them).
// explicit_call: an entry point of the engine's own (tgp_logpdf_adjoint_group_sde, DESIGN 4.14; tgp_posterior_rand_group_sde, DESIGN 4.15), served under TGP_OPT_SWEEP >= 1 as sweep_group_eligible's.
bool sweep_group_sde_eligible(const tgp_handle* h, uint32_t flags, bool explicit_call = false) {
    if (h->opt_sweep < (explicit_call ? 1 : 2) || h->sweep_state < 0 || h->is_dense || h->p != 1 || h->ordering != 0 || !h->sde) return false;
    if (h->d < tgp_sweep::kGroupMinD || h->d > tgp_sweep::kGroupMaxD) return false;
    if ((flags & TGP_REUSE_REDUCE) || h->opt_chunk != 0 || h->variant_opt != 0 || !h->opt_steady2 || h->opt_graph != 0) return false;
    if (h->T < tgp_sweep::kGroupMinT || h->mv.T != h->T || h->mv.sH != 0 || h->sweepm.empty()) return false;
    return h->sde_closed && h->opt_sde_closed && !h->sde_coef_host.empty() && h->mv.sa == 0;
}

// The tile sweep (tgp_sweep_tile.hip, DESIGN 4.16): sweep_group_eligible's conditions at 9 <= d <= 16, LTI form, under TGP_OPT_SWEEP = 2 only -- no (d, call)
// pair is routed here by default (profiles/sweep_tile_time.txt has the medians beside the general engine's: a routing change would rest on them).  A
// fully observed series with one noise variance is the wide engine's (tgp_wide.hip) and, where that declines, the general engine's as before.
bool sweep_tile_eligible(const tgp_handle* h, uint32_t flags, const uint8_t* missing) {
    if (h->opt_sweep < 2 || h->sweep_state < 0 || h->is_dense || h->p != 1 || h->ordering != 0 || h->sde) return false;
    if (h->d < tgp_sweep::kTileMinD || h->d > tgp_sweep::kTileMaxD) return false;
    if (missing == nullptr && h->mv.sR == 0) return false;
    if ((flags & TGP_REUSE_REDUCE) || h->opt_chunk != 0 || h->variant_opt != 0 || !h->opt_steady2 || h->opt_graph != 0) return false;
    if (h->T < tgp_sweep::kTileMinT || h->mv.T != h->T || h->mv.sH != 0 || h->sweepm.empty()) return false;
    return h->mv.sA == 0 && h->mv.sa == 0 && h->mv.sQ == 0;
}

// The host model the plans of both engines read, from the staged blocks of the bound model.  record_pinf: the stationary covariance of an SDE-described
// model is the one tgp_model_set_sde took (the closed-form record; tgp_model_set_x0 may have replaced the prior since) -- the adjoint calls and the group
// sweep's draw.  tgp_logpdf, the posterior calls and the lane sweep's draw pass none: the bound x0P stands for Pinf.  (The plans read Pinf, coef and
// tau_typ of SDE-described models only: tgp_sweep_plan.hpp.)
tgp_sweep::ModelHost sweep_host_model(const tgp_handle* h, bool record_pinf) {
    const int d = h->d;
    const size_t dd = (size_t)d * d;
    const double* q = h->sweepm.data();
    tgp_sweep::ModelHost mh;
    mh.d = d;
    mh.sde = h->sde;
    mh.A = h->sde ? h->sde_A1Q1_host.data() : q;
    mh.a = q + dd;
    mh.Q = h->sde ? h->sde_A1Q1_host.data() + dd : q + dd + d;
    mh.H = q + 2 * dd + d;
    mh.hh = q[2 * dd + 2 * d];
    mh.R = h->sweep_Rrep;
    mh.x0m = h->x0m.data();
    mh.x0P = h->x0P.data();
    mh.coef = h->sde ? h->sde_coef_host.data() : nullptr;
    if (h->sde && record_pinf) mh.Pinf = h->sde_coef_host.data() + d + 2 * dd;
    mh.tau_typ = h->sweep_tau;
    return mh;
}

// The call kinds of the sweep engines.  Each has a second warm-up of its own beside the forward W -- the smoother's Wb, the draw's Wd, the adjoint's
// Wa --, remembered apart on the handle, forced by TGP_OPT_SWEEP_WARMUP_BACK and reported in the backward slots of tgp_sweep_info.
enum class SweepKind { marginals = 0, draw = 1, adjoint = 2 };      // (marginals: logpdf alone, or with the posterior marginals)
int& sweep_back_slot(tgp_handle* h, SweepKind kind) { return kind == SweepKind::draw ? h->sweep_Wd : kind == SweepKind::adjoint ? h->sweep_Wa : h->sweep_Wb; }
// per kind: the tag and the slot's name in the TGP_STEADY_DEBUG lines; why a call with status bit 4 / bit 8 is declined (null: a silent decline)
const struct { const char *tag, *slot, *not_pd, *not_finite; } kSweepKindText[3] = {
    {"", "Wb", nullptr, nullptr},
    {" draw", "Wd", "a Cholesky pivot of the draw is not positive", "non-finite values in the draw"},
    {" adjoint", "Wa", "an innovation variance is not positive", "non-finite values in the pass"}};

// What sweep_attempts needs of an engine: the lane sweep (tgp_sweep.hip, d <= 4), the group sweep (tgp_sweep_group.hip, 5 <= d <= 8) and the tile sweep
// (tgp_sweep_tile.hip, 9 <= d <= 16) behind one call sequence.  Plain function pointers on the handle, three static instances (no allocation on the call path).  Wk: the kind's second warm-up; post: a
// marginals call asks for the posterior marginals.
struct SweepOps {
    const char* tag;       // in the TGP_STEADY_DEBUG lines
    const char* name;      // in the entry points' error texts
    const char* (*kname)(const tgp_handle* h, SweepKind kind, bool post);
    // (creates the engine at the first call; with the handle's forced geometry)
    bool (*plan)(tgp_handle* h, const tgp_sweep::ModelHost& mh, SweepKind kind, bool post, int W, int Wk, std::string* why);
    int (*enqueue)(tgp_handle* h, const tgp_sweep::Call& c, const char** kname, std::string* err);
    double (*finish)(tgp_handle* h, SweepKind kind, int* status, int* w, int* wk, double* dist_f, double* dist_k);      // (a draw: returns 0)
    void (*geometry)(tgp_handle* h, int* C, int64_t* nwaves);
    // behind finish of an adjoint call whose status is clean.  so (null: the LTI form, to o): the sums over the closed form's coefficients
    void (*adjoint_blocks)(tgp_handle* h, const tgp_sweep::ModelHost& mh, const tgp_sweep::AdjointOut& o, const tgp_sweep::AdjointSdeOut* so);
};

// The lane sweep has a slot per kind in plan, finish and force_geometry: the forced and the repaired second warm-up go to the kind's own, and a draw or
// an adjoint plans beside the Wb the bound model remembers.
const SweepOps kLaneSweep = {
    "sweep", "sweep engine",
    [](const tgp_handle* h, SweepKind kind, bool post) {
        if (kind == SweepKind::adjoint) return h->sde ? tgp_sweep::adjoint_sde_kernel_name() : tgp_sweep::adjoint_kernel_name();
        return tgp_sweep::kernel_name(h->d, h->sde, post, kind == SweepKind::draw);
    },
    [](tgp_handle* h, const tgp_sweep::ModelHost& mh, SweepKind kind, bool, int W, int Wk, std::string* why) {
        if (!h->sweep) h->sweep = tgp_sweep::create();
        int forced[3] = {0, 0, 0}, hint[3] = {h->sweep_Wb, 0, 0};
        forced[(int)kind] = h->sweep_fWb;
        hint[(int)kind] = Wk;
        tgp_sweep::force_geometry(h->sweep, h->sweep_fC, h->sweep_fW, forced[0], forced[1], forced[2]);
        return tgp_sweep::plan(h->sweep, mh, h->T, W, hint[0], h->num_cu, why, hint[1], hint[2]);
    },
    [](tgp_handle* h, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep::enqueue(h->sweep, h->stream, c, kname, err); },
    [](tgp_handle* h, SweepKind kind, int* status, int* w, int* wk, double* df, double* dk) {
        int* ran[3] = {nullptr, nullptr, nullptr};
        ran[(int)kind] = wk;
        const double lml = tgp_sweep::finish(h->sweep, status, w, ran[0], df, dk, ran[1], ran[2]);
        return kind == SweepKind::draw ? 0.0 : lml;
    },
    [](tgp_handle* h, int* C, int64_t* nw) { tgp_sweep::geometry(h->sweep, C, nullptr, nullptr, nw); },
    [](tgp_handle* h, const tgp_sweep::ModelHost&, const tgp_sweep::AdjointOut& o, const tgp_sweep::AdjointSdeOut* so) {
        if (so) tgp_sweep::adjoint_blocks_sde(h->sweep, *so);
        else tgp_sweep::adjoint_blocks(h->sweep, o);
    }};

// The group sweep has one backward slot: a draw and an adjoint run on the posterior call's geometry with their warm-up in it, and say so by a flag.
// Its SDE adjoint pulls step 0 back on the host through the first transition of the host model.
const SweepOps kGroupSweep = {
    "sweep group", "group sweep",
    [](const tgp_handle* h, SweepKind kind, bool post) {
        if (kind == SweepKind::adjoint) return h->sde ? tgp_sweep_group::adjoint_sde_kernel_name() : tgp_sweep_group::adjoint_kernel_name();
        return kind == SweepKind::draw ? tgp_sweep_group::draw_kernel_name(h->sde) : tgp_sweep_group::kernel_name(post, h->sde);
    },
    [](tgp_handle* h, const tgp_sweep::ModelHost& mh, SweepKind kind, bool post, int W, int Wk, std::string* why) {
        if (!h->sweep_group) h->sweep_group = tgp_sweep_group::create();
        tgp_sweep_group::force_geometry(h->sweep_group, h->sweep_fC, h->sweep_fW, h->sweep_fWb);
        return tgp_sweep_group::plan(h->sweep_group, mh, h->T, W, Wk, h->num_cu, post || kind != SweepKind::marginals, why, kind == SweepKind::adjoint,
                                     kind == SweepKind::draw);
    },
    [](tgp_handle* h, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep_group::enqueue(h->sweep_group, h->stream, c, kname, err); },
    [](tgp_handle* h, SweepKind kind, int* status, int* w, int* wk, double* df, double* dk) {
        const double lml = tgp_sweep_group::finish(h->sweep_group, status, w, wk, df, dk);
        return kind == SweepKind::draw ? 0.0 : lml;
    },
    [](tgp_handle* h, int* C, int64_t* nw) { tgp_sweep_group::geometry(h->sweep_group, C, nullptr, nullptr, nw); },
    [](tgp_handle* h, const tgp_sweep::ModelHost& mh, const tgp_sweep::AdjointOut& o, const tgp_sweep::AdjointSdeOut* so) {
        if (so) tgp_sweep_group::adjoint_blocks_sde(h->sweep_group, mh, *so);
        else tgp_sweep_group::adjoint_blocks(h->sweep_group, o);
    }};

// The tile sweep serves marginals calls (logpdf, posterior marginals) and the adjoint gradient (DESIGN 4.17): one backward slot -- an adjoint runs on the
// posterior call's geometry with its warm-up Wa in it -- and the draw (DESIGN 4.18) the same way with its warm-up Wd.
const SweepOps kTileSweep = {
    "sweep tile", "tile sweep",
    [](const tgp_handle*, SweepKind kind, bool post) {
        if (kind == SweepKind::draw) return tgp_sweep_tile::draw_kernel_name();
        return kind == SweepKind::adjoint ? tgp_sweep_tile::adjoint_kernel_name() : tgp_sweep_tile::kernel_name(post);
    },
    [](tgp_handle* h, const tgp_sweep::ModelHost& mh, SweepKind kind, bool post, int W, int Wk, std::string* why) {
        if (!h->sweep_tile) h->sweep_tile = tgp_sweep_tile::create();
        tgp_sweep_tile::force_geometry(h->sweep_tile, h->sweep_fC, h->sweep_fW, h->sweep_fWb);
        return tgp_sweep_tile::plan(h->sweep_tile, mh, h->T, W, Wk, h->num_cu, post || kind != SweepKind::marginals, why);
    },
    [](tgp_handle* h, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep_tile::enqueue(h->sweep_tile, h->stream, c, kname, err); },
    [](tgp_handle* h, SweepKind kind, int* status, int* w, int* wk, double* df, double* dk) {
        const double lml = tgp_sweep_tile::finish(h->sweep_tile, status, w, wk, df, dk);
        return kind == SweepKind::draw ? 0.0 : lml;
    },
    [](tgp_handle* h, int* C, int64_t* nw) { tgp_sweep_tile::geometry(h->sweep_tile, C, nullptr, nullptr, nw); },
    [](tgp_handle* h, const tgp_sweep::ModelHost&, const tgp_sweep::AdjointOut& o, const tgp_sweep::AdjointSdeOut*) { tgp_sweep_tile::adjoint_blocks(h->sweep_tile, o); }};

// Runs a call on one of the sweep engines: staging ONCE, up to four attempts with doubled warm-ups, the engine switched off for the bound model where it
// cannot serve it.  What a kind brings:
//   stage(tm)   inputs and outputs staged in front of the attempts (a host-resident series is not uploaded again by every retry); marks tm.inputs_done()
//   fill(c)     the kind's fields of the engine's call record (the series, mask, per-step streams and gaps are filled here)
//   deliver()   behind a clean status alone: the outputs reach the caller's memory, with the synchronisation they need
// *served = false: the engine declined, nothing reached the caller's memory.  why == nullptr: declines are silent, the caller goes on to the general
// engine; else *why says what a draw or a gradient was declined for.
template <class Stage, class Fill, class Deliver>
int sweep_attempts(tgp_handle* h, const SweepOps& eng, SweepKind kind, bool post, const tgp_sweep::ModelHost& mh, double* lml_out, bool* served, std::string* why,
                   Stage&& stage, Fill&& fill, Deliver&& deliver) {
    *served = false;
    static const bool dbg = getenv("TGP_STEADY_DEBUG") != nullptr;
    const auto& text = kSweepKindText[(int)kind];
    auto decline = [&](const char* because) {
        if (why) *why = because;
        return TGP_OK;
    };
    const bool forced = h->sweep_fW || h->sweep_fWb || h->sweep_fC;
    int& back = sweep_back_slot(h, kind);
    int W = h->sweep_W, Wk = back;
    for (int64_t& v : h->sweep_info) v = 0;
    auto replan = [&]() {
        std::string w;
        if (eng.plan(h, mh, kind, post, W, Wk, &w)) return true;
        if (dbg) fprintf(stderr, "[tgp %s%s] does not apply: %s\n", eng.tag, text.tag, w.c_str());
        h->sweep_state = -1;
        decline(("the sweep engine's plan declines the model (" + w + ")").c_str());
        return false;
    };
    if (!replan()) return TGP_OK;
    CallTimer tm(h, /*clear=*/false);
    TRY(stage(tm));
    const char* const kname0 = eng.kname(h, kind, post);
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (attempt > 0 && !replan()) return TGP_OK;
        tgp_sweep::Call c;
        c.T = h->T;
        c.y = h->mv.y;
        c.mask = h->mv.missing;
        c.R = h->mv.sR != 0 ? h->mv.R : nullptr;
        c.hh = h->mv.sh != 0 ? h->mv.h : nullptr;
        c.tau = h->sde ? h->btau.d() : nullptr;
        fill(c);
        {
            std::string err;
            const char* kname = kname0;
            LaunchScope ls(h, kname);
            if (eng.enqueue(h, c, &kname, &err) != 0) return h->fail(TGP_EHIP, err);
        }
        tm.kernels_done();
        if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
        HIPCHK(hipStreamSynchronize(h->stream));
        resolve_profile(h);
        int status = 0, w = 0, wk = 0;
        const double lml = eng.finish(h, kind, &status, &w, &wk, &h->sweep_dist[0], &h->sweep_dist[1]);
        int C = 0;
        int64_t nw = 0;
        eng.geometry(h, &C, &nw);
        h->sweep_info[1] = C; h->sweep_info[2] = w; h->sweep_info[3] = wk; h->sweep_info[4] = nw; h->sweep_info[5] = attempt + 1; h->sweep_info[6] = status;
        if (dbg)
            fprintf(stderr, "[tgp %s%s] attempt %d: C %d W %d %s %d waves %lld status %d dist %.3g / %.3g\n", eng.tag, text.tag, attempt, C, w, text.slot, wk, (long long)nw,
                    status, h->sweep_dist[0], h->sweep_dist[1]);
        if (status & 12) {      // not positive definite / non-finite values: the general engine (the evaluated route, the tangent scans) reports it the way it always has
            if (status & 4) h->sweep_state = -1;      // (a property of the model, not of this series: later calls do not pay for a launch that cannot serve them)
            return decline((status & 4) ? text.not_pd : text.not_finite);
        }
        if (status & 3) {       // a warm-up was too short: longer ones (a forced geometry is a test's: report, do not repair)
            if (forced) return decline("a warm-up of the forced geometry is too short (tgp_sweep_info)");
            if (status & 1) W = 2 * w;
            if (status & 2) Wk = 2 * wk;
            continue;
        }
        TRY(deliver());
        read_timing(h);
        note_served(h, Served::sweep, 0, lml, lml_out);
        h->sweep_W = w;
        back = wk;
        h->sweep_state = 1;
        h->sweep_info[0] = 1;
        *served = true;
        return TGP_OK;
    }
    h->sweep_state = -1;      // four attempts, warm-ups still too short: a model that mixes too slowly for this engine
    return decline("the warm-ups stayed too short over four attempts");
}

// logpdf / posterior marginals on the lane sweep (d <= 4; LTI and SDE form) or, sweep_group_call, on the group sweep (5 <= d <= 8; LTI form, and SDE form
// where sweep_group_sde_eligible says so).  Rnew is staged only where the marginals are asked for; the kernel writes straight to the caller's device
// arrays or their staging.  A decline is silent (nothing the caller must undo): the caller goes on to the general engine.
int sweep_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, double* mean_out, double* var_out,
               double* lml_out, bool* served, const SweepOps& eng = kLaneSweep) {
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0, rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    const void* pR = nullptr;
    double *dm = nullptr, *dv = nullptr;
    return sweep_attempts(
        h, eng, SweepKind::marginals, mean_out != nullptr, sweep_host_model(h, /*record_pinf=*/false), lml_out, served, nullptr,
        [&](CallTimer& tm) -> int {
            if (mean_out) TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
            TRY(set_obs(h, y, missing, flags));
            tm.inputs_done();
            TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
            TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
            return TGP_OK;
        },
        [&](tgp_sweep::Call& c) {
            c.Rnew = static_cast<const double*>(pR);
            c.rnew_per_step = (mean_out && !rshared) ? 1 : 0;
            c.mean = dm;
            c.var = dv;
        },
        [&]() -> int {
            TRY(copy_back(h, mean_out, dm, nT, odev));
            TRY(copy_back(h, var_out, dv, nT, odev));
            if (mean_out && !odev) HIPCHK(hipStreamSynchronize(h->stream));
            return TGP_OK;
        });
}
int sweep_group_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, double* mean_out, double* var_out,
                     double* lml_out, bool* served) {
    return sweep_call(h, y, missing, flags, Rnew, mean_out, var_out, lml_out, served, kGroupSweep);
}

// rand of the posterior on the lane sweep (k_sweep_draw, DESIGN 4.7; LTI and SDE form) or on the group sweep (k_sweep_group_draw, DESIGN 4.12;
// k_sweep_group_draw_sde, 4.15) or on the tile sweep (k_sweep_tile_draw, DESIGN 4.18).  The draw goes to the handle's own buffer and reaches y_out behind the checks: a declined call (*served = false, *why
// set) leaves a device y_out untouched as well.  The lane sweep's draw plans an SDE-described model from the bound x0P, the group sweep's from the
// record's Pinf, so that a prior replaced by tgp_model_set_x0 is served (as the adjoint calls').
int sweep_draw_call(tgp_handle* h, const SweepOps& eng, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, const double* eps_t,
                    const double* eps_e, const double* eps_0, double* y_out, bool* served, std::string* why) {
    const int d = h->d;
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0, rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    const void *pR = nullptr, *pet = nullptr, *pee = nullptr;
    double* dy = nullptr;
    return sweep_attempts(
        h, eng, SweepKind::draw, /*post=*/true, sweep_host_model(h, /*record_pinf=*/&eng == &kGroupSweep), nullptr, served, why,
        [&](CallTimer& tm) -> int {
            TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
            TRY(set_obs(h, y, missing, flags));
            TRY(stage_in(h, h->beps_t, eps_t, (size_t)h->T * d * sizeof(double), idev, &pet));
            TRY(stage_in(h, h->beps_e, eps_e, nT, idev, &pee));
            tm.inputs_done();
            HIPCHK(h->bo1.ensure(nT));
            dy = h->bo1.d();
            return TGP_OK;
        },
        [&](tgp_sweep::Call& c) {
            c.Rnew = static_cast<const double*>(pR);
            c.rnew_per_step = rshared ? 0 : 1;
            c.eps_t = static_cast<const double*>(pet);
            c.eps_e = static_cast<const double*>(pee);
            for (int k = 0; k < d; ++k) c.eps_0[k] = eps_0[k];
            c.y_out = dy;
        },
        [&]() -> int {
            HIPCHK(hipMemcpyAsync(y_out, dy, nT, odev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
            HIPCHK(hipStreamSynchronize(h->stream));
            return TGP_OK;
        });
}

// The adjoint gradient on the lane sweep (k_sweep_adjoint, DESIGN 4.8; k_sweep_adjoint_sde, 4.9) or on the group sweep (k_sweep_group_adjoint, DESIGN 4.11;
// k_sweep_group_adjoint_sde, 4.14).  The per-step gradients go to the handle's own buffers and reach gh_steps / gR_steps behind the checks, the block
// gradients are written behind them too: *served = false with *why set: the engine declined, no output was written.
// so (null: the LTI form, the block gradients go to o): an SDE-described model -- the sums over the closed form's coefficients go to *so, `o` is unused.
int sweep_adjoint_call(tgp_handle* h, const SweepOps& eng, const double* y, const uint8_t* missing, uint32_t flags, double* lml_out, const tgp_sweep::AdjointOut& o,
                       const tgp_sweep::AdjointSdeOut* so, double* gh_steps, double* gR_steps, bool* served, std::string* why) {
    const bool odev = (flags & TGP_OUT_DEVICE) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    const tgp_sweep::ModelHost mh = sweep_host_model(h, /*record_pinf=*/true);
    double *dgh = nullptr, *dgR = nullptr;
    return sweep_attempts(
        h, eng, SweepKind::adjoint, /*post=*/true, mh, lml_out, served, why,
        [&](CallTimer& tm) -> int {
            TRY(set_obs(h, y, missing, flags));
            tm.inputs_done();
            if (gh_steps) {
                HIPCHK(h->bo1.ensure(nT));
                dgh = h->bo1.d();
            }
            if (gR_steps) {
                HIPCHK(h->bo2.ensure(nT));
                dgR = h->bo2.d();
            }
            return TGP_OK;
        },
        [&](tgp_sweep::Call& c) {
            c.adjoint = true;
            c.gh_steps = dgh;
            c.gR_steps = dgR;
        },
        [&]() -> int {
            if (gh_steps) HIPCHK(hipMemcpyAsync(gh_steps, dgh, nT, odev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
            if (gR_steps) HIPCHK(hipMemcpyAsync(gR_steps, dgR, nT, odev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
            if (gh_steps || gR_steps) HIPCHK(hipStreamSynchronize(h->stream));
            eng.adjoint_blocks(h, mh, o, so);
            return TGP_OK;
        });
}

// d logpdf / d F from the sums over the closed form's coefficients: the transpose of sde_closed_form's map.  coef = [lam d | N d*d | N^2 / 2 d*d | ...];
// a connected component S of n rows has N = F_SS + lam I, lam = -tr F_SS / n:  gN = [n >= 2] gN1_SS + [n >= 3] (gN2_SS N' + N' gN2_SS) / 2,
// gF_SS = gN - ((sum_S gl_i + tr gN) / n) I.  Entries outside the components are zero (the closed form does not read them).
void sde_coef_to_gF(int d, const double* coef, const double* gl, const double* gN1, const double* gN2, double* gF) {
    const double* N = coef + d;
    std::vector<int> comp(d);
    for (int i = 0; i < d; ++i) comp[i] = i;
    auto find = [&](int i) { while (comp[i] != i) i = comp[i] = comp[comp[i]]; return i; };
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i)
            if (i != j && N[i + j * d] != 0.0) comp[find(i)] = find(j);      // (off the diagonal N is F: the same components)
    for (int i = 0; i < d * d; ++i) gF[i] = 0.0;
    std::vector<char> seen(d, 0);
    for (int r = 0; r < d; ++r) {
        const int root = find(r);
        if (seen[root]) continue;
        seen[root] = 1;
        std::vector<int> S;
        for (int i = 0; i < d; ++i)
            if (find(i) == root) S.push_back(i);
        const int n = (int)S.size();
        std::vector<double> gN((size_t)n * n, 0.0);
        for (int jj = 0; jj < n; ++jj)
            for (int ii = 0; ii < n; ++ii) {
                double v = n >= 2 ? gN1[S[ii] + S[jj] * d] : 0.0;
                if (n >= 3)
                    for (int k = 0; k < n; ++k)
                        v += 0.5 * (gN2[S[ii] + S[k] * d] * N[S[jj] + S[k] * d] + N[S[k] + S[ii] * d] * gN2[S[k] + S[jj] * d]);
                gN[ii + jj * n] = v;
            }
        double tr = 0.0;
        for (int ii = 0; ii < n; ++ii) tr += gl[S[ii]] + gN[ii + ii * n];
        for (int jj = 0; jj < n; ++jj)
            for (int ii = 0; ii < n; ++ii) gF[S[ii] + S[jj] * d] = gN[ii + jj * n] - (ii == jj ? tr / n : 0.0);
    }
}

// The outputs of tgp_logpdf_adjoint_sde / tgp_logpdf_adjoint_group_sde from an engine's record (any output null).  A model bound without A1 took
// A1 = E (I + N1 + N2), E = diag(e^(-lam_i)), at step 0: its G_0 (so.gA1) belongs to the coefficients, with tau = 1, and gA1 is zero.
struct SdeGrads {      // (the entries' output arguments, in their order)
    double *gF, *gPinf, *gA1, *ga, *gH, *ghh, *gR, *gx0m, *gx0P;
};
void sde_adjoint_outputs(const tgp_handle* h, const tgp_sweep::AdjointSdeOut& so, const SdeGrads& g) {
    const int d = h->d, dd = d * d;
    const double* coef = h->sde_coef_host.data();
    if (!h->have_AQ1) {
        const double* A1 = h->sde_A1Q1_host.data();
        for (int i = 0; i < d; ++i) {
            const double e = std::exp(-coef[i]);
            double s = 0.0;
            for (int j = 0; j < d; ++j) {
                s += so.gA1[i + j * d] * A1[i + j * d];
                so.gN1[i + j * d] += e * so.gA1[i + j * d];
                so.gN2[i + j * d] += e * so.gA1[i + j * d];
            }
            so.gl[i] -= s;
        }
        for (int i = 0; i < dd; ++i) so.gA1[i] = 0.0;
    }
    if (g.gF) sde_coef_to_gF(d, coef, so.gl, so.gN1, so.gN2, g.gF);
    if (g.gPinf) std::memcpy(g.gPinf, so.gPinf, sizeof(double) * dd);
    if (g.gA1) std::memcpy(g.gA1, so.gA1, sizeof(double) * dd);
    if (g.ga) std::memcpy(g.ga, so.ga, sizeof(double) * d);
    if (g.gH) std::memcpy(g.gH, so.gH, sizeof(double) * d);
    if (g.ghh) *g.ghh = *so.ghh;
    if (g.gR) *g.gR = *so.gR;
    if (g.gx0m) std::memcpy(g.gx0m, so.gx0m, sizeof(double) * d);
    if (g.gx0P) std::memcpy(g.gx0P, so.gx0P, sizeof(double) * dd);
}

bool steady2_served(tgp_handle* h) {
    const bool ran = h->host_result[6] == tgp_steady::kStatusRan;
    h->steady2_state = ran ? 1 : -1;
    if (ran) h->served = Served::steady2;
    return ran;
}

