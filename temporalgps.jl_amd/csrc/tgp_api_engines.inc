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
// shared) with sweep_group_eligible's others.  tgp_logpdf and tgp_[logpdf_and_]posterior_marginals only (the gradient and the draw decline: the
// predicate above), and under TGP_OPT_SWEEP = 2 only: no (d, call) pair is routed here by default (profiles/sweep_group_sde_time.txt has the measured medians
// beside the general engine's: a routing change would rest on them).
bool sweep_group_sde_eligible(const tgp_handle* h, uint32_t flags) {
    if (h->opt_sweep < 2 || h->sweep_state < 0 || h->is_dense || h->p != 1 || h->ordering != 0 || !h->sde) return false;
    if (h->d < tgp_sweep::kGroupMinD || h->d > tgp_sweep::kGroupMaxD) return false;
    if ((flags & TGP_REUSE_REDUCE) || h->opt_chunk != 0 || h->variant_opt != 0 || !h->opt_steady2 || h->opt_graph != 0) return false;
    if (h->T < tgp_sweep::kGroupMinT || h->mv.T != h->T || h->mv.sH != 0 || h->sweepm.empty()) return false;
    return h->sde_closed && h->opt_sde_closed && !h->sde_coef_host.empty() && h->mv.sa == 0;
}

// The host model the plans of both engines read, from the staged blocks of the bound model
tgp_sweep::ModelHost sweep_host_model(const tgp_handle* h) {
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
    mh.tau_typ = h->sweep_tau;
    return mh;
}

// What sweep_run needs of an engine: the lane sweep (tgp_sweep.hip) and the group sweep (tgp_sweep_group.hip) behind one call sequence.  Plain function
// pointers on the handle (no allocation on the call path); `post`: the call asks for the posterior marginals.
struct SweepEngineOps {
    const char* tag;
    const char* kname;
    bool post;
    bool (*plan)(tgp_handle* h, const tgp_sweep::ModelHost& mh, bool post, int W, int Wb, std::string* why);      // (with the handle's forced geometry)
    int (*enqueue)(tgp_handle* h, const tgp_sweep::Call& c, const char** kname, std::string* err);
    double (*finish)(tgp_handle* h, int* status, int* w, int* wb, double* dist_f, double* dist_b);
    void (*geometry)(tgp_handle* h, int* C, int64_t* nwaves);
};

// Runs a logpdf / posterior call on one of the sweep engines: staging ONCE, up to four attempts with doubled warm-ups, the engine switched off for the
// bound model where it cannot serve it.  *served = false: it declined (nothing the caller must undo); the caller goes on to the general engine.
int sweep_run(tgp_handle* h, const SweepEngineOps& eng, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, double* mean_out,
              double* var_out, double* lml_out, bool* served) {
    *served = false;
    static const bool dbg = getenv("TGP_STEADY_DEBUG") != nullptr;
    const tgp_sweep::ModelHost mh = sweep_host_model(h);
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0;
    const bool rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    int W = h->sweep_W, Wb = h->sweep_Wb;
    for (int64_t& v : h->sweep_info) v = 0;
    // inputs and outputs are staged ONCE, in front of the attempts (round-5 advice: a host-resident series was uploaded again by every retry)
    {
        std::string why;
        if (!eng.plan(h, mh, eng.post, W, Wb, &why)) {
            if (dbg) fprintf(stderr, "[tgp %s] does not apply: %s\n", eng.tag, why.c_str());
            h->sweep_state = -1;
            return TGP_OK;
        }
    }
    CallTimer tm(h, /*clear=*/false);
    const void* pR = nullptr;
    if (mean_out) TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
    TRY(set_obs(h, y, missing, flags));
    tm.inputs_done();
    double *dm = nullptr, *dv = nullptr;
    TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
    TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (attempt > 0) {
            std::string why;
            if (!eng.plan(h, mh, eng.post, W, Wb, &why)) {
                if (dbg) fprintf(stderr, "[tgp %s] does not apply: %s\n", eng.tag, why.c_str());
                h->sweep_state = -1;
                return TGP_OK;
            }
        }
        tgp_sweep::Call c;
        c.T = h->T;
        c.y = h->mv.y;
        c.mask = h->mv.missing;
        c.R = h->mv.sR != 0 ? h->mv.R : nullptr;
        c.hh = h->mv.sh != 0 ? h->mv.h : nullptr;
        c.tau = h->sde ? h->btau.d() : nullptr;
        c.Rnew = static_cast<const double*>(pR);
        c.rnew_per_step = (mean_out && !rshared) ? 1 : 0;
        c.mean = dm;
        c.var = dv;
        {
            std::string err;
            const char* kname = eng.kname;
            LaunchScope ls(h, kname);
            if (eng.enqueue(h, c, &kname, &err) != 0) return h->fail(TGP_EHIP, err);
        }
        tm.kernels_done();
        if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
        HIPCHK(hipStreamSynchronize(h->stream));
        resolve_profile(h);
        int status = 0, w = 0, wb = 0;
        const double lml = eng.finish(h, &status, &w, &wb, &h->sweep_dist[0], &h->sweep_dist[1]);
        int C = 0;
        int64_t nw = 0;
        eng.geometry(h, &C, &nw);
        h->sweep_info[1] = C; h->sweep_info[2] = w; h->sweep_info[3] = wb; h->sweep_info[4] = nw; h->sweep_info[5] = attempt + 1; h->sweep_info[6] = status;
        if (dbg) fprintf(stderr, "[tgp %s] attempt %d: C %d W %d Wb %d waves %lld status %d dist %.3g / %.3g\n", eng.tag, attempt, C, w, wb, (long long)nw, status, h->sweep_dist[0], h->sweep_dist[1]);
        if (status & 12) {      // not positive definite / non-finite values: the general engine reports it the way it always has
            if (status & 4) h->sweep_state = -1;      // (a property of the model, not of this series: later calls do not pay for a launch that cannot serve them)
            return TGP_OK;
        }
        if (status & 3) {       // a warm-up was too short: longer ones (a forced geometry is a test's: report, do not repair)
            if (h->sweep_fW || h->sweep_fWb || h->sweep_fC) return TGP_OK;
            if (status & 1) W = 2 * w;
            if (status & 2) Wb = 2 * wb;
            continue;
        }
        TRY(copy_back(h, mean_out, dm, nT, odev));
        TRY(copy_back(h, var_out, dv, nT, odev));
        if ((mean_out && !odev)) HIPCHK(hipStreamSynchronize(h->stream));
        read_timing(h);
        note_served(h, Served::sweep, 0, lml, lml_out);
        h->sweep_W = w;
        h->sweep_Wb = wb;
        h->sweep_state = 1;
        h->sweep_info[0] = 1;
        *served = true;
        return TGP_OK;
    }
    h->sweep_state = -1;      // four attempts, warm-ups still too short: a model that mixes too slowly for this engine
    return TGP_OK;
}

// The lane sweep (d <= 4; LTI and SDE form)
int sweep_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, double* mean_out, double* var_out,
               double* lml_out, bool* served) {
    if (!h->sweep) h->sweep = tgp_sweep::create();
    const SweepEngineOps eng = {
        "sweep", tgp_sweep::kernel_name(h->d, h->sde, mean_out != nullptr), mean_out != nullptr,
        [](tgp_handle* hh, const tgp_sweep::ModelHost& mh, bool, int W, int Wb, std::string* why) {
            tgp_sweep::force_geometry(hh->sweep, hh->sweep_fC, hh->sweep_fW, hh->sweep_fWb);
            return tgp_sweep::plan(hh->sweep, mh, hh->T, W, Wb, hh->num_cu, why);
        },
        [](tgp_handle* hh, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep::enqueue(hh->sweep, hh->stream, c, kname, err); },
        [](tgp_handle* hh, int* status, int* w, int* wb, double* df, double* db) { return tgp_sweep::finish(hh->sweep, status, w, wb, df, db); },
        [](tgp_handle* hh, int* C, int64_t* nw) { tgp_sweep::geometry(hh->sweep, C, nullptr, nullptr, nw); }};
    return sweep_run(h, eng, y, missing, flags, Rnew, mean_out, var_out, lml_out, served);
}

// The group sweep (5 <= d <= 8; LTI form, and SDE form where sweep_group_sde_eligible says so)
int sweep_group_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, double* mean_out, double* var_out,
                     double* lml_out, bool* served) {
    if (!h->sweep_group) h->sweep_group = tgp_sweep_group::create();
    const SweepEngineOps eng = {
        "sweep group", tgp_sweep_group::kernel_name(mean_out != nullptr, h->sde), mean_out != nullptr,
        [](tgp_handle* hh, const tgp_sweep::ModelHost& mh, bool post, int W, int Wb, std::string* why) {
            tgp_sweep_group::force_geometry(hh->sweep_group, hh->sweep_fC, hh->sweep_fW, hh->sweep_fWb);
            return tgp_sweep_group::plan(hh->sweep_group, mh, hh->T, W, Wb, hh->num_cu, post, why);
        },
        [](tgp_handle* hh, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep_group::enqueue(hh->sweep_group, hh->stream, c, kname, err); },
        [](tgp_handle* hh, int* status, int* w, int* wb, double* df, double* db) { return tgp_sweep_group::finish(hh->sweep_group, status, w, wb, df, db); },
        [](tgp_handle* hh, int* C, int64_t* nw) { tgp_sweep_group::geometry(hh->sweep_group, C, nullptr, nullptr, nw); }};
    return sweep_run(h, eng, y, missing, flags, Rnew, mean_out, var_out, lml_out, served);
}

// What sweep_draw_run needs of an engine: the lane sweep's draw kernel and the group sweep's behind one call sequence (SweepAdjointOps' twin; Wd: the draw's
// warm-up, in the lane engine's draw slot and the group engine's backward slot).
struct SweepDrawOps {
    const char* tag;
    const char* kname;
    bool (*plan)(tgp_handle* h, const tgp_sweep::ModelHost& mh, int W, int Wd, std::string* why);      // (with the handle's forced geometry)
    int (*enqueue)(tgp_handle* h, const tgp_sweep::Call& c, const char** kname, std::string* err);
    void (*finish)(tgp_handle* h, int* status, int* w, int* wd, double* dist_f, double* dist_d);
    void (*geometry)(tgp_handle* h, int* C, int64_t* nwaves);
};

// rand of the posterior on one of the sweep engines: sweep_run's staging and repair loop around a draw kernel.  The draw pass sits in the backward slots
// of tgp_sweep_info (its warm-up Wd is remembered apart from Wb; TGP_OPT_SWEEP_WARMUP_BACK forces it here).  *served = false with *why set: the engine
// declined, nothing was written to y_out.
int sweep_draw_run(tgp_handle* h, const SweepDrawOps& eng, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, const double* eps_t,
                   const double* eps_e, const double* eps_0, double* y_out, bool* served, std::string* why) {
    *served = false;
    static const bool dbg = getenv("TGP_STEADY_DEBUG") != nullptr;
    const int d = h->d;
    const tgp_sweep::ModelHost mh = sweep_host_model(h);
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0;
    const bool rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    const bool forced = h->sweep_fW || h->sweep_fWb || h->sweep_fC;
    int W = h->sweep_W, Wd = h->sweep_Wd;
    for (int64_t& v : h->sweep_info) v = 0;
    auto replan = [&]() {
        std::string w;
        if (eng.plan(h, mh, W, Wd, &w)) return true;
        if (dbg) fprintf(stderr, "[tgp %s] does not apply: %s\n", eng.tag, w.c_str());
        h->sweep_state = -1;
        *why = "the sweep engine's plan declines the model (" + w + ")";
        return false;
    };
    if (!replan()) return TGP_OK;
    // inputs and the output are staged ONCE, in front of the attempts.  The draw goes to the handle's own buffer and reaches y_out behind the checks:
    // a declined call leaves a device y_out untouched as well.
    CallTimer tm(h, /*clear=*/false);
    const void *pR = nullptr, *pet = nullptr, *pee = nullptr;
    TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
    TRY(set_obs(h, y, missing, flags));
    TRY(stage_in(h, h->beps_t, eps_t, (size_t)h->T * d * sizeof(double), idev, &pet));
    TRY(stage_in(h, h->beps_e, eps_e, nT, idev, &pee));
    tm.inputs_done();
    HIPCHK(h->bo1.ensure(nT));
    double* dy = h->bo1.d();
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (attempt > 0 && !replan()) return TGP_OK;
        tgp_sweep::Call c;
        c.T = h->T;
        c.y = h->mv.y;
        c.mask = h->mv.missing;
        c.R = h->mv.sR != 0 ? h->mv.R : nullptr;
        c.hh = h->mv.sh != 0 ? h->mv.h : nullptr;
        c.tau = h->sde ? h->btau.d() : nullptr;
        c.Rnew = static_cast<const double*>(pR);
        c.rnew_per_step = rshared ? 0 : 1;
        c.eps_t = static_cast<const double*>(pet);
        c.eps_e = static_cast<const double*>(pee);
        for (int k = 0; k < d; ++k) c.eps_0[k] = eps_0[k];
        c.y_out = dy;
        {
            std::string err;
            const char* kname = eng.kname;
            LaunchScope ls(h, kname);
            if (eng.enqueue(h, c, &kname, &err) != 0) return h->fail(TGP_EHIP, err);
        }
        tm.kernels_done();
        if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
        HIPCHK(hipStreamSynchronize(h->stream));
        resolve_profile(h);
        int status = 0, w = 0, wd = 0;
        eng.finish(h, &status, &w, &wd, &h->sweep_dist[0], &h->sweep_dist[1]);
        int C = 0;
        int64_t nw = 0;
        eng.geometry(h, &C, &nw);
        h->sweep_info[1] = C; h->sweep_info[2] = w; h->sweep_info[3] = wd; h->sweep_info[4] = nw; h->sweep_info[5] = attempt + 1; h->sweep_info[6] = status;
        if (dbg) fprintf(stderr, "[tgp %s] attempt %d: C %d W %d Wd %d waves %lld status %d dist %.3g / %.3g\n", eng.tag, attempt, C, w, wd, (long long)nw, status, h->sweep_dist[0], h->sweep_dist[1]);
        if (status & 12) {      // not positive definite / non-finite values: the evaluated route reports it the way it always has
            if (status & 4) h->sweep_state = -1;
            *why = (status & 4) ? "a Cholesky pivot of the draw is not positive" : "non-finite values in the draw";
            return TGP_OK;
        }
        if (status & 3) {       // a warm-up was too short: longer ones (a forced geometry is a test's: report, do not repair)
            if (forced) {
                *why = "a warm-up of the forced geometry is too short (tgp_sweep_info)";
                return TGP_OK;
            }
            if (status & 1) W = 2 * w;
            if (status & 2) Wd = 2 * wd;
            continue;
        }
        if (odev) HIPCHK(hipMemcpyAsync(y_out, dy, nT, hipMemcpyDeviceToDevice, h->stream));
        else HIPCHK(hipMemcpyAsync(y_out, dy, nT, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        read_timing(h);
        note_served(h, Served::sweep, 0, 0.0, nullptr);
        h->sweep_W = w;
        h->sweep_Wd = wd;
        h->sweep_state = 1;
        h->sweep_info[0] = 1;
        *served = true;
        return TGP_OK;
    }
    h->sweep_state = -1;      // four attempts, warm-ups still too short: a model that mixes too slowly for this engine
    *why = "the warm-ups stayed too short over four attempts";
    return TGP_OK;
}

// The draw on the lane sweep (k_sweep_draw, DESIGN 4.7; LTI and SDE form)
int sweep_draw_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, const double* eps_t, const double* eps_e,
                    const double* eps_0, double* y_out, bool* served, std::string* why) {
    *served = false;
    if (!h->sweep) h->sweep = tgp_sweep::create();
    const SweepDrawOps eng = {
        "sweep draw", tgp_sweep::kernel_name(h->d, h->sde, true, true),
        [](tgp_handle* hh, const tgp_sweep::ModelHost& m, int W, int Wd, std::string* w) {
            tgp_sweep::force_geometry(hh->sweep, hh->sweep_fC, hh->sweep_fW, 0, hh->sweep_fWb);
            return tgp_sweep::plan(hh->sweep, m, hh->T, W, hh->sweep_Wb, hh->num_cu, w, Wd);
        },
        [](tgp_handle* hh, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep::enqueue(hh->sweep, hh->stream, c, kname, err); },
        [](tgp_handle* hh, int* status, int* w, int* wd, double* df, double* dd) { (void)tgp_sweep::finish(hh->sweep, status, w, nullptr, df, dd, wd); },
        [](tgp_handle* hh, int* C, int64_t* nw) { tgp_sweep::geometry(hh->sweep, C, nullptr, nullptr, nw); }};
    return sweep_draw_run(h, eng, y, missing, flags, Rnew, eps_t, eps_e, eps_0, y_out, served, why);
}

// The same at 5 <= d <= 8 on the group sweep (k_sweep_group_draw, DESIGN 4.12; LTI form): the posterior call's geometry with Wd in its backward slot.
int sweep_group_draw_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, const double* Rnew, const double* eps_t,
                          const double* eps_e, const double* eps_0, double* y_out, bool* served, std::string* why) {
    *served = false;
    if (!h->sweep_group) h->sweep_group = tgp_sweep_group::create();
    const SweepDrawOps eng = {
        "sweep group draw", tgp_sweep_group::draw_kernel_name(),
        [](tgp_handle* hh, const tgp_sweep::ModelHost& m, int W, int Wd, std::string* w) {
            tgp_sweep_group::force_geometry(hh->sweep_group, hh->sweep_fC, hh->sweep_fW, hh->sweep_fWb);
            return tgp_sweep_group::plan(hh->sweep_group, m, hh->T, W, Wd, hh->num_cu, /*post=*/true, w, /*adjoint=*/false, /*draw=*/true);
        },
        [](tgp_handle* hh, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep_group::enqueue(hh->sweep_group, hh->stream, c, kname, err); },
        [](tgp_handle* hh, int* status, int* w, int* wd, double* df, double* dd) { (void)tgp_sweep_group::finish(hh->sweep_group, status, w, wd, df, dd); },
        [](tgp_handle* hh, int* C, int64_t* nw) { tgp_sweep_group::geometry(hh->sweep_group, C, nullptr, nullptr, nw); }};
    return sweep_draw_run(h, eng, y, missing, flags, Rnew, eps_t, eps_e, eps_0, y_out, served, why);
}

// What sweep_adjoint_run needs of an engine: the lane sweep's adjoint kernels and the group sweep's behind one call sequence (SweepEngineOps' twin; Wa: the
// adjoint's warm-up, in the engines' backward slot).
struct SweepAdjointOps {
    const char* tag;
    const char* kname;
    bool (*plan)(tgp_handle* h, const tgp_sweep::ModelHost& mh, int W, int Wa, std::string* why);      // (with the handle's forced geometry)
    int (*enqueue)(tgp_handle* h, const tgp_sweep::Call& c, const char** kname, std::string* err);
    double (*finish)(tgp_handle* h, int* status, int* w, int* wa, double* dist_f, double* dist_b);
    void (*geometry)(tgp_handle* h, int* C, int64_t* nwaves);
};

// The adjoint gradient on one of the sweep engines: sweep_run's staging and repair loop around an adjoint kernel.  The adjoint pass sits in the backward
// slots of tgp_sweep_info (its warm-up Wa is remembered apart from Wb and Wd; TGP_OPT_SWEEP_WARMUP_BACK forces it here).  The per-step gradients go to the
// handle's own buffers and reach gh_steps / gR_steps behind the checks, the block gradients are written behind them too (write_blocks):
// *served = false with *why set: the engine declined, no output was written.
template <class WriteBlocks>
int sweep_adjoint_run(tgp_handle* h, const SweepAdjointOps& eng, const tgp_sweep::ModelHost& mh, bool sde, const double* y, const uint8_t* missing, uint32_t flags,
                      double* lml_out, double* gh_steps, double* gR_steps, bool* served, std::string* why, WriteBlocks&& write_blocks) {
    *served = false;
    static const bool dbg = getenv("TGP_STEADY_DEBUG") != nullptr;
    const bool odev = (flags & TGP_OUT_DEVICE) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    const bool forced = h->sweep_fW || h->sweep_fWb || h->sweep_fC;
    int W = h->sweep_W, Wa = h->sweep_Wa;
    for (int64_t& v : h->sweep_info) v = 0;
    auto replan = [&]() {
        std::string w;
        if (eng.plan(h, mh, W, Wa, &w)) return true;
        if (dbg) fprintf(stderr, "[tgp %s] does not apply: %s\n", eng.tag, w.c_str());
        h->sweep_state = -1;
        *why = "the sweep engine's plan declines the model (" + w + ")";
        return false;
    };
    if (!replan()) return TGP_OK;
    CallTimer tm(h, /*clear=*/false);
    TRY(set_obs(h, y, missing, flags));
    tm.inputs_done();
    double *dgh = nullptr, *dgR = nullptr;
    if (gh_steps) {
        HIPCHK(h->bo1.ensure(nT));
        dgh = h->bo1.d();
    }
    if (gR_steps) {
        HIPCHK(h->bo2.ensure(nT));
        dgR = h->bo2.d();
    }
    for (int attempt = 0; attempt < 4; ++attempt) {
        if (attempt > 0 && !replan()) return TGP_OK;
        tgp_sweep::Call c;
        c.T = h->T;
        c.y = h->mv.y;
        c.mask = h->mv.missing;
        c.R = h->mv.sR != 0 ? h->mv.R : nullptr;
        c.hh = h->mv.sh != 0 ? h->mv.h : nullptr;
        c.tau = sde ? h->btau.d() : nullptr;
        c.adjoint = true;
        c.gh_steps = dgh;
        c.gR_steps = dgR;
        {
            std::string err;
            const char* kname = eng.kname;
            LaunchScope ls(h, kname);
            if (eng.enqueue(h, c, &kname, &err) != 0) return h->fail(TGP_EHIP, err);
        }
        tm.kernels_done();
        if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
        HIPCHK(hipStreamSynchronize(h->stream));
        resolve_profile(h);
        int status = 0, w = 0, wa = 0;
        const double lml = eng.finish(h, &status, &w, &wa, &h->sweep_dist[0], &h->sweep_dist[1]);
        int C = 0;
        int64_t nw = 0;
        eng.geometry(h, &C, &nw);
        h->sweep_info[1] = C; h->sweep_info[2] = w; h->sweep_info[3] = wa; h->sweep_info[4] = nw; h->sweep_info[5] = attempt + 1; h->sweep_info[6] = status;
        if (dbg) fprintf(stderr, "[tgp %s] attempt %d: C %d W %d Wa %d waves %lld status %d dist %.3g / %.3g\n", eng.tag, attempt, C, w, wa, (long long)nw, status, h->sweep_dist[0], h->sweep_dist[1]);
        if (status & 12) {      // not positive definite / non-finite values: the tangent scans report it the way they always have
            if (status & 4) h->sweep_state = -1;
            *why = (status & 4) ? "an innovation variance is not positive" : "non-finite values in the pass";
            return TGP_OK;
        }
        if (status & 3) {       // a warm-up was too short: longer ones (a forced geometry is a test's: report, do not repair)
            if (forced) {
                *why = "a warm-up of the forced geometry is too short (tgp_sweep_info)";
                return TGP_OK;
            }
            if (status & 1) W = 2 * w;
            if (status & 2) Wa = 2 * wa;
            continue;
        }
        if (gh_steps) HIPCHK(hipMemcpyAsync(gh_steps, dgh, nT, odev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
        if (gR_steps) HIPCHK(hipMemcpyAsync(gR_steps, dgR, nT, odev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
        if (gh_steps || gR_steps) HIPCHK(hipStreamSynchronize(h->stream));
        write_blocks();
        read_timing(h);
        note_served(h, Served::sweep, 0, lml, lml_out);
        h->sweep_W = w;
        h->sweep_Wa = wa;
        h->sweep_state = 1;
        h->sweep_info[0] = 1;
        *served = true;
        return TGP_OK;
    }
    h->sweep_state = -1;      // four attempts, warm-ups still too short: a model that mixes too slowly for this engine
    *why = "the warm-ups stayed too short over four attempts";
    return TGP_OK;
}

// The adjoint gradient on the lane sweep (k_sweep_adjoint, DESIGN 4.8; LTI form).
// so (null: the LTI form): an SDE-described model -- k_sweep_adjoint_sde (DESIGN 4.9), the sums over the closed form's coefficients go to *so and `o` is unused.
int sweep_adjoint_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, double* lml_out, const tgp_sweep::AdjointOut& o,
                       double* gh_steps, double* gR_steps, bool* served, std::string* why, const tgp_sweep::AdjointSdeOut* so = nullptr) {
    *served = false;
    if (!h->sweep) h->sweep = tgp_sweep::create();
    const int d = h->d;
    const size_t dd = (size_t)d * d;
    const double* q = h->sweepm.data();
    tgp_sweep::ModelHost mh;
    mh.d = d;
    mh.sde = so != nullptr;
    mh.A = so ? h->sde_A1Q1_host.data() : q;
    mh.a = q + dd;
    mh.Q = so ? h->sde_A1Q1_host.data() + dd : q + dd + d;
    mh.H = q + 2 * dd + d;
    mh.hh = q[2 * dd + 2 * d];
    mh.R = h->sweep_Rrep;
    mh.x0m = h->x0m.data();
    mh.x0P = h->x0P.data();
    if (so) {      // (the stationary covariance as tgp_model_set_sde took it: tgp_model_set_x0 may have replaced the prior since)
        mh.coef = h->sde_coef_host.data();
        mh.Pinf = h->sde_coef_host.data() + d + 2 * dd;
        mh.tau_typ = h->sweep_tau;
    }
    const SweepAdjointOps eng = {
        "sweep adjoint", so ? tgp_sweep::adjoint_sde_kernel_name() : tgp_sweep::adjoint_kernel_name(),
        [](tgp_handle* hh, const tgp_sweep::ModelHost& m, int W, int Wa, std::string* w) {
            tgp_sweep::force_geometry(hh->sweep, hh->sweep_fC, hh->sweep_fW, 0, 0, hh->sweep_fWb);
            return tgp_sweep::plan(hh->sweep, m, hh->T, W, hh->sweep_Wb, hh->num_cu, w, 0, Wa);
        },
        [](tgp_handle* hh, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep::enqueue(hh->sweep, hh->stream, c, kname, err); },
        [](tgp_handle* hh, int* status, int* w, int* wa, double* df, double* db) { return tgp_sweep::finish(hh->sweep, status, w, nullptr, df, db, nullptr, wa); },
        [](tgp_handle* hh, int* C, int64_t* nw) { tgp_sweep::geometry(hh->sweep, C, nullptr, nullptr, nw); }};
    return sweep_adjoint_run(h, eng, mh, so != nullptr, y, missing, flags, lml_out, gh_steps, gR_steps, served, why, [&]() {
        if (so) tgp_sweep::adjoint_blocks_sde(h->sweep, *so);
        else tgp_sweep::adjoint_blocks(h->sweep, o);
    });
}

// The same at 5 <= d <= 8 on the group sweep (k_sweep_group_adjoint, DESIGN 4.11; LTI form): the posterior call's geometry with Wa in its backward slot.
int sweep_group_adjoint_call(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, double* lml_out, const tgp_sweep::AdjointOut& o,
                             double* gh_steps, double* gR_steps, bool* served, std::string* why) {
    *served = false;
    if (!h->sweep_group) h->sweep_group = tgp_sweep_group::create();
    const SweepAdjointOps eng = {
        "sweep group adjoint", tgp_sweep_group::adjoint_kernel_name(),
        [](tgp_handle* hh, const tgp_sweep::ModelHost& m, int W, int Wa, std::string* w) {
            tgp_sweep_group::force_geometry(hh->sweep_group, hh->sweep_fC, hh->sweep_fW, hh->sweep_fWb);
            return tgp_sweep_group::plan(hh->sweep_group, m, hh->T, W, Wa, hh->num_cu, /*post=*/true, w, /*adjoint=*/true);
        },
        [](tgp_handle* hh, const tgp_sweep::Call& c, const char** kname, std::string* err) { return tgp_sweep_group::enqueue(hh->sweep_group, hh->stream, c, kname, err); },
        [](tgp_handle* hh, int* status, int* w, int* wa, double* df, double* db) { return tgp_sweep_group::finish(hh->sweep_group, status, w, wa, df, db); },
        [](tgp_handle* hh, int* C, int64_t* nw) { tgp_sweep_group::geometry(hh->sweep_group, C, nullptr, nullptr, nw); }};
    return sweep_adjoint_run(h, eng, sweep_host_model(h), false, y, missing, flags, lml_out, gh_steps, gR_steps, served, why,
                             [&]() { tgp_sweep_group::adjoint_blocks(h->sweep_group, o); });
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

bool steady2_served(tgp_handle* h) {
    const bool ran = h->host_result[6] == tgp_steady::kStatusRan;
    h->steady2_state = ran ? 1 : -1;
    if (ran) h->served = Served::steady2;
    return ran;
}

