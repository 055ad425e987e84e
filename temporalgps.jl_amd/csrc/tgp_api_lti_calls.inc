// Part of tgp_api.hip (included there, one translation unit): the LTI one-launch calls behind the entry points: adjoint, filter, smoother / posterior draw, pair statistic.
static int ensure_pinned(tgp_handle* h, size_t need) {
    if (need <= h->flt_cap) return TGP_OK;
    if (h->flt_host) (void)tgp_alloc::host_free(h->flt_host);
    h->flt_host = nullptr;
    h->flt_cap = 0;
    if (tgp_alloc::host_malloc(reinterpret_cast<void**>(&h->flt_host), need * sizeof(double), hipHostMallocDefault) != hipSuccess) return h->fail(TGP_EHIP, "hipHostMalloc");
    h->flt_cap = need;
    return TGP_OK;
}

// The adjoint pass in ONE launch (d <= 6): plan and head on the host (tgp_plan::build_filter / filter_head: the covariance half, the head's
// forward recursion from its few observations), forward and reverse recursions + the sums behind the head in k_adjoint_one, the head's
// reverse part and the sweep through the covariance recursion in tgp_adjoint::finish as before.  *served = false: the five-launch form runs.
static int adjoint_lti_call(tgp_handle* h, const double* y, uint32_t flags, double* lml_out, const tgp_adjoint::Out& o, bool* served) {
    *served = false;
    tgp_plan::ModelHost mh;
    if (!h->opt_modal || chunk_engine_requested(h) || h->is_dense || !h->lti || h->p != 1 || h->ordering != 0 || h->sde || h->d > tgp_powers::kAdjointMaxD || !modal_host_model(h, mh)) return TGP_OK;
    tgp_plan::FilterPlan fp;
    tgp_powers::plan_filter(mh, h->T, fp);
    if (fp.why != tgp_plan::kOk) return TGP_OK;
    const long long nwg = tgp_powers::adjoint_workgroups(fp, h->T);
    if (nwg < 1) return TGP_OK;
    const int d = h->d, ns = tgp_powers::adjoint_sums(d);
    const size_t dd = (size_t)d * d, nhs = (size_t)fp.nhs, nrec = tgp_adjoint::record_size(d);
    const size_t need = nhs + (size_t)nwg * ns + d + nrec + 16;
    TRY(ensure_pinned(h, need));
    double *yh = h->flt_host, *part = yh + nhs, *psi = part + (size_t)nwg * ns, *rec = psi + d;
    if (!h->sm_sync) {
        if (tgp_alloc::host_malloc(reinterpret_cast<void**>(&h->sm_sync), 32 * sizeof(double), hipHostMallocDefault) != hipSuccess) return h->fail(TGP_EHIP, "hipHostMalloc");
        std::memset(h->sm_sync, 0, 32 * sizeof(double));
    }
    CallTimer tm(h, /*clear=*/false);
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    // The head beside the kernel (DESIGN 3.15): the launch goes first, workgroup 0 hands the head's observations over through pinned memory,
    // the host answers with the head's end state.  With synchronous launches: copy, synchronise, head, launch.
    const bool overlap = tgp_modal::overlap_allowed();
    double* mu_end = h->sm_sync;
    long long* sflag = reinterpret_cast<long long*>(h->sm_sync + 16);
    const long long seq = ++h->smooth_seq;
    double quad_head = 0.0;
    tgp_powers::HeadHandover hh;
    if (overlap) {
        hh.head_in = yh;
        hh.head_in_flag = sflag;
        hh.mu0 = mu_end;
        hh.mu0_flag = sflag + 1;
        hh.seq = seq;
    } else {
        HIPCHK(hipMemcpyAsync(yh, h->mv.y, nhs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(hipStreamSynchronize(h->stream));
        tgp_powers::plan_filter_head(mh, fp, yh, nullptr, nullptr, mu_end, &quad_head);
    }
    {
        LaunchScope ls(h, "k_adjoint_one");
        const int rc = tgp_powers::adjoint_lti(h->stream, fp, overlap ? nullptr : mu_end, h->mv.y, h->T, part, psi, overlap ? &hh : nullptr);
        if (rc != 0) return h->fail(TGP_EHIP, std::string("tgp_logpdf_adjoint: launch: ") + hipGetErrorString((hipError_t)rc));
    }
    bool handshake_ok = true;
    if (overlap) {
        handshake_ok = tgp_modal::await_host_flag(sflag, 2 * seq, h->stream);
        if (handshake_ok) tgp_powers::plan_filter_head(mh, fp, yh, nullptr, nullptr, mu_end, &quad_head);
        __atomic_store_n(sflag + 1, 2 * seq, __ATOMIC_RELEASE);      // (also when the hand-over failed: workgroup 0 never waits for what will not come)
    }
    tm.kernels_done();
    if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    resolve_profile(h);
    if (!handshake_ok) return h->fail(TGP_EHIP, "tgp_logpdf_adjoint: the host / device hand-over timed out");
    // the record tgp_adjoint::finish reads: the sums (fixed order over the workgroups), psi at the head's end, n0 / T, the model blocks
    for (size_t e = 0; e < nrec; ++e) rec[e] = 0.0;
    for (long long g = 0; g < nwg; ++g)
        for (int e = 0; e < ns; ++e) rec[e] += part[(size_t)g * ns + e];
    for (int i = 0; i < d; ++i) rec[ns + i] = psi[i];
    double* meta = rec + ns + 2 * d;
    meta[0] = (double)fp.n0;
    meta[1] = 0.0;
    meta[2] = (double)h->T;
    meta[3] = 1.0;
    double* md = meta + 4;
    std::memcpy(md, h->hostm.data(), (2 * dd + 2 * d + 2) * sizeof(double));
    double* x0 = md + 2 * dd + 2 * d + 2;
    for (int i = 0; i < d; ++i) x0[i] = h->x0m[i];
    for (int c = 0; c < d; ++c)
        for (int r = 0; r <= c; ++r) x0[d + c * (c + 1) / 2 + r] = h->x0P[r + (size_t)c * d];
    if (tgp_adjoint::finish(d, rec, yh, (int64_t)nhs, o, (int64_t)nhs) != 0) return h->fail(TGP_EHIP, "tgp_logpdf_adjoint: inconsistent record");
    note_served(h, Served::dense, fp.n0, head_lml(fp, h->T, quad_head, rec[dd + 3 * d + 1]), lml_out);
    *served = true;
    return TGP_OK;
}

// The adjoint pass of a wide LTI model (8 < d <= 63, every block shared, one noise variance, no per-step emission offsets; tgp_wide::adjoint): the
// wide-state engine's forward kernel, its backward kernel in the ADJ form and the sums k_wide_gram on the device, the head and the host half of the
// gradient (tgp_wide_adjoint_host.hpp) on the host.  *served = false: the engine does not apply (nothing the caller must undo).
static int wide_adjoint_call(tgp_handle* h, const double* y, uint32_t flags, double* lml_out, const tgp_adjoint::Out& o, bool* served) {
    *served = false;
    if (h->wide_ht != nullptr) return TGP_OK;
    if (!h->wide) h->wide = tgp_wide::create();
    tgp_wide::ModelHost mh;
    wide_host_model(h, mh);
    if (!tgp_wide::plan(h->wide, mh, h->T)) {
        h->wide_state = -1;
        return TGP_OK;
    }
    CallTimer tm(h, /*clear=*/false);
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    std::string err;
    double lml = 0.0;
    bool declined = true;
    {
        const std::string nm_k = std::string("k_wide_adjoint: ") + tgp_wide::kernel_name(h->wide) + " + k_wide_bwd + k_wide_gram";
        LaunchScope ls(h, nm_k.c_str());
        if (tgp_wide::adjoint(h->wide, h->stream, mh, h->T, h->mv.y, &lml, o, &declined, &err) != 0) return h->fail(TGP_EHIP, err);
    }
    if (declined) return TGP_OK;
    if (h->profile) HIPCHK(hipStreamSynchronize(h->stream));      // (the bracket's closing event)
    resolve_profile(h);
    if (getenv("TGP_STEADY_DEBUG") != nullptr) {
        const tgp_wide::Info& in = tgp_wide::last_plan(h->wide);
        fprintf(stderr, "[tgp wide adjoint] n0 %d halo %d chunks %lld x %lld steps, plan %.3f ms, host finish %.3f ms\n", in.n0, in.halo, in.chunks, in.chunk_len, in.plan_ms,
                in.finish_ms);
    }
    note_served(h, Served::wide, tgp_wide::last_plan(h->wide).n0, lml, lml_out);
    *served = true;
    return TGP_OK;
}

int tgp_logpdf_adjoint(tgp_handle* h, const double* y, uint32_t flags, double* lml_out, double* gA, double* ga, double* gQ, double* gH,
                       double* ghh, double* gR, double* gx0m, double* gx0P) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (y != nullptr) {
        bool served = false;
        const tgp_adjoint::Out o1{gA, ga, gQ, gH, ghh, gR, gx0m, gx0P};
        TRY(adjoint_lti_call(h, y, flags, lml_out, o1, &served));
        if (served) return TGP_OK;
    }
    const int keep_state = h->steady2_state;
    h->steady2_state = 0;            // (an earlier "does not apply" verdict of a posterior call -- series shorter than head + tail -- does not bind this one)
    const bool ok = steady2_eligible(h, nullptr, flags);
    h->steady2_state = keep_state;
    if (!ok && wide_eligible(h, y, nullptr)) {
        bool served = false;
        const tgp_adjoint::Out ow{gA, ga, gQ, gH, ghh, gR, gx0m, gx0P};
        TRY(wide_adjoint_call(h, y, flags, lml_out, ow, &served));
        if (served) return TGP_OK;
    }
    if (!ok)
        return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint: Forward LTI models (every block shared), one noise variance, scalar observations, d <= 8 "
                                         "(the stationary-gain engine) or 8 < d <= 63 (the wide-state engine, no per-step emission offsets); use "
                                         "tgp_logpdf_grad otherwise");
    constexpr int64_t kHead = (int64_t)tgp_steady::kHeadMaxTiles * tgp_steady::kTile;
    const size_t nrec = tgp_steady::grad_record_size(h->d);
    const int64_t nyh = h->T < kHead ? h->T : kHead;
    if (!h->adj_host && tgp_alloc::host_malloc(reinterpret_cast<void**>(&h->adj_host), (tgp_steady::grad_record_size(tgp_steady::kMaxD) + kHead) * sizeof(double), hipHostMallocDefault) != hipSuccess)
        return h->fail(TGP_EHIP, "hipHostMalloc");
    CallTimer tm(h, /*clear=*/false);
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    TRY(steady2_enqueue(h, nullptr, false, nullptr, nullptr, true));
    tm.kernels_done();
    HIPCHK(hipMemcpyAsync(h->adj_host, tgp_steady::grad_record(h->steady2), nrec * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipMemcpyAsync(h->adj_host + nrec, h->mv.y, (size_t)nyh * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    TRY(tm.finish(lml_out));
    if (h->host_result[6] != tgp_steady::kStatusRan)
        return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint: the filter covariance of this model does not settle within the head (or the series is shorter "
                                         "than the head); use tgp_logpdf_grad");
    const tgp_adjoint::Out o{gA, ga, gQ, gH, ghh, gR, gx0m, gx0P};
    if (tgp_adjoint::finish(h->d, h->adj_host, h->adj_host + nrec, nyh, o) != 0) return h->fail(TGP_EHIP, "tgp_logpdf_adjoint: inconsistent record");
    return TGP_OK;
}

// _filter of an LTI model (Forward, scalar observations, one noise variance, no missing data, d <= 6): the head on the host from its few
// observations, everything behind it in ONE kernel (tgp_powers::filter_lti; DESIGN 3.13).  *served = false: the caller runs the general engine.
static int filter_lti_call(tgp_handle* h, const double* y, uint32_t flags, double* m_out, double* P_out, double* lml_out, bool* served) {
    *served = false;
    tgp_plan::ModelHost mh;
    if (!h->opt_modal || chunk_engine_requested(h) || h->is_dense || !h->lti || h->p != 1 || h->ordering != 0 || h->sde || h->d > tgp_plan::kRandMaxD || !modal_host_model(h, mh)) return TGP_OK;
    tgp_plan::FilterPlan fp;
    tgp_powers::plan_filter(mh, h->T, fp);
    if (fp.why != tgp_plan::kOk) return TGP_OK;
    const int d = h->d;
    const size_t dd = (size_t)d * d, nhs = (size_t)fp.nhs;
    const long long nwg = tgp_powers::filter_workgroups(fp, h->T);
    const size_t need = nhs * (1 + d + dd) + (size_t)nwg + 8;
    TRY(ensure_pinned(h, need));
    double *yh = h->flt_host, *mh_out = yh + nhs, *Ph_out = mh_out + nhs * d, *part = Ph_out + nhs * dd;
    const bool odev = (flags & TGP_OUT_DEVICE) != 0;
    const size_t nm = (size_t)h->T * d * sizeof(double), nP = nm * d;
    CallTimer tm(h, /*clear=*/false);
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    HIPCHK(hipMemcpyAsync(yh, h->mv.y, nhs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    double mu_end[tgp_plan::kRandMaxD], quad_head = 0.0;
    tgp_powers::plan_filter_head(mh, fp, yh, m_out ? mh_out : nullptr, P_out ? Ph_out : nullptr, mu_end, &quad_head);
    double *dm = nullptr, *dP = nullptr;
    TRY(stage_out(h, h->bo1, m_out, nm, odev, &dm));
    TRY(stage_out(h, h->bo2, P_out, nP, odev, &dP));
    if (dm) HIPCHK(hipMemcpyAsync(dm, mh_out, nhs * d * sizeof(double), hipMemcpyHostToDevice, h->stream));
    if (dP) HIPCHK(hipMemcpyAsync(dP, Ph_out, nhs * dd * sizeof(double), hipMemcpyHostToDevice, h->stream));
    {
        LaunchScope ls(h, "k_filter_one");
        const int rc = tgp_powers::filter_lti(h->stream, fp, mu_end, h->mv.y, h->T, dm, dP, part);
        if (rc != 0) return h->fail(TGP_EHIP, std::string("tgp_filter: launch: ") + hipGetErrorString((hipError_t)rc));
    }
    tm.kernels_done();
    TRY(copy_back(h, m_out, dm, nm, odev));
    TRY(copy_back(h, P_out, dP, nP, odev));
    if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    resolve_profile(h);
    double ssq = 0.0;
    for (long long g = 0; g < nwg; ++g) ssq += part[g];
    note_served(h, Served::dense, fp.n0, head_lml(fp, h->T, quad_head, ssq), lml_out);
    *served = true;
    return TGP_OK;
}

// logpdf + posterior marginals of an LTI model WITHOUT a modal form (Forward, scalar observations, one noise variance, no missing data,
// d <= 8; a defective closed loop: two summands with one length scale, ...): the head on the host, everything behind it in ONE kernel on the
// dense powers of the closed loop and of the settled reverse-time transition (tgp_powers::smooth_lti, DESIGN 3.15).  *served = false: the
// five-launch engine runs the call.
// Every block shared but the emission offset: a GP with a mean function on a regular grid (lti_sde.jl:118-131).  The gains never see the offset, so the
// stationary structure holds; the dense-powers kernel subtracts it per step (SmoothCall::hh_t).
static bool lti_but_offset(const tgp_handle* h) {
    return !h->lti && !h->is_dense && !h->sde && h->p == 1 && h->ordering == 0 && h->mv.sA == 0 && h->mv.sa == 0 && h->mv.sQ == 0 && h->mv.sH == 0 && h->mv.sR == 0 &&
           h->mv.sh != 0 && h->mv.T == h->T && !h->sweepm.empty() && h->opt_steady2 && h->opt_chunk == 0;
}
static int smooth_lti_call(tgp_handle* h, const double* y, uint32_t flags, const double* Rnew, double* mean_out, double* var_out, double* lml_out, bool* served,
                           const SmoothRand* rnd) {
    *served = false;
    tgp_plan::ModelHost mh;
    const bool offs = lti_but_offset(h);
    if (offs && h->opt_modal && !rnd) {      // (the plans read the shared blocks the sweep engine's record holds: the same layout as hostm)
        const int d = h->d;
        const size_t dd = (size_t)d * d;
        const double* q = h->sweepm.data();
        mh.d = d;
        mh.A = q; mh.a = q + dd; mh.Q = q + dd + d; mh.H = q + 2 * dd + d; mh.hh = q + 2 * dd + 2 * d; mh.R = q + 2 * dd + 2 * d + 1;
        mh.x0m = h->x0m.data();
        mh.x0P = h->x0P.data();
    }
    if (!h->opt_modal || h->smooth_state < 0 || chunk_engine_requested(h) || h->is_dense || !(h->lti || (offs && !rnd)) || h->p != 1 || h->ordering != 0 || h->sde ||
        h->d > tgp_plan::kRandMaxD || (!offs && !modal_host_model(h, mh)) || (!rnd && (mean_out != nullptr) != (var_out != nullptr)) || (mean_out && !Rnew))
        return TGP_OK;
    if (rnd && (h->d > tgp_powers::kSmoothRandMaxD || !mean_out || var_out || !rnd->eps_t || !rnd->eps_e || !rnd->eps_0)) return TGP_OK;
    const bool post = mean_out != nullptr;      // (false: logpdf only -- the forward half alone, no halo behind a span)
    constexpr size_t HM = tgp_plan::kHeadMax;
    const size_t nwg_max = (size_t)(h->T / 1024) + 2;
    TRY(ensure_pinned(h, 14 * HM + nwg_max + tgp_plan::kTailMax + 8));
    // hin: y | Rnew (| eta | eps [nhs][d <= 6] of a draw) of the head, its emission offsets at 10 nhs; hout: mean | var
    double *hin = h->flt_host, *hout = hin + 12 * HM, *tvb = hout + 2 * HM, *part = tvb + tgp_plan::kTailMax;
    if (!h->sm_sync) {
        if (tgp_alloc::host_malloc(reinterpret_cast<void**>(&h->sm_sync), 32 * sizeof(double), hipHostMallocDefault) != hipSuccess) return h->fail(TGP_EHIP, "hipHostMalloc");
        std::memset(h->sm_sync, 0, 32 * sizeof(double));
    }
    double *mu_end = h->sm_sync, *xi = h->sm_sync + 8;
    long long* sflag = reinterpret_cast<long long*>(h->sm_sync + 16);      // [0] head inputs on the host, [1] mu_end, [2] xi, [3] head outputs
    tgp_plan::SmoothPlan sp;
    tgp_powers::plan_smooth(mh, h->T, sp, tvb, post);
    if (sp.why != tgp_plan::kOk) {
        if (post) h->smooth_state = -1;      // (a function of the model and T alone: the next call need not ask again)
        return TGP_OK;
    }
    const tgp_plan::FilterPlan& fp = sp.fp;
    const size_t nhs = (size_t)fp.nhs;
    const long long nwg = tgp_powers::smooth_workgroups(sp, h->T, post);
    if (nwg < 1 || (size_t)nwg > nwg_max) return TGP_OK;
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0, rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    // The head BESIDE the kernel (tgp_powers.hpp SmoothCall): the launch goes first; workgroup 0 hands the head's inputs to the host through
    // pinned memory, the host answers with the head's end state, runs the head backwards once workgroup 0 has raised xi, and the last workgroup
    // writes the head's outputs: one launch, one synchronisation, no copy on any stream in between.  With synchronous launches: the same
    // steps one after the other, copies on the handle's stream.
    const bool overlap = tgp_modal::overlap_allowed();
    const long long seq = ++h->smooth_seq;
    double rU[tgp_powers::kSmoothRandMaxD * tgp_powers::kSmoothRandMaxD], rv0[tgp_powers::kSmoothRandMaxD], rs0 = 0.0;
    if (rnd && !tgp_powers::plan_smooth_rand_factors(sp, rnd->eps_0, rU, rv0, &rs0)) return TGP_OK;      // (a noise factor not positive definite: the evaluated route gives the verdict)
    CallTimer tm(h, /*clear=*/false);
    const void *pR = nullptr, *pet = nullptr, *pee = nullptr;
    if (post) TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
    if (rnd) {
        TRY(stage_in(h, h->beps_t, rnd->eps_t, (size_t)h->T * h->d * sizeof(double), idev, &pet));
        TRY(stage_in(h, h->beps_e, rnd->eps_e, nT, idev, &pee));
    }
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    double *dm = nullptr, *dv = nullptr;
    TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
    TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
    double quad_head = 0.0;
    const bool hand = idev || offs;      // the kernel hands the head's inputs over (a per-step offset lives on the device whatever the call's arrays are)
    const double *yhead = hand ? hin : y, *rnhead = hand ? hin + nhs : Rnew;
    const double* hhhead = offs ? hin + 10 * nhs : nullptr;
    const double *eehead = rnd ? (hand ? hin + 2 * nhs : rnd->eps_e) : nullptr, *ethead = rnd ? (hand ? hin + 3 * nhs : rnd->eps_t) : nullptr;
    tgp_powers::SmoothCall c;
    c.T = h->T;
    c.y = h->mv.y;
    c.Rnew = static_cast<const double*>(pR);
    c.rnew_per_step = rshared ? 0 : 1;
    c.tvb = tvb;
    c.mean = dm;
    c.var = dv;
    c.part = part;
    c.xi_out = xi;
    c.seq = seq;
    c.hh_t = offs ? h->mv.h : nullptr;
    if (rnd) {
        c.eps_t = static_cast<const double*>(pet);
        c.eps_e = static_cast<const double*>(pee);
        c.U = rU;
        c.v0 = rv0;
        c.s0 = rs0;
    }
    if (overlap) {
        if (hand) {
            c.head_in = hin;
            c.head_in_flag = sflag;
        }
        c.mu0 = mu_end;
        c.mu0_flag = sflag + 1;
        if (post) {
            c.xi_flag = sflag + 2;
            c.head_out = hout;
            c.head_out_flag = sflag + 3;
        }
    } else {
        if (hand) {
            HIPCHK(hipMemcpyAsync(hin, h->mv.y, nhs * sizeof(double), hipMemcpyDeviceToHost, h->stream));      // (the staged copies: device whatever the call's arrays are)
            if (post) HIPCHK(hipMemcpyAsync(hin + nhs, pR, (rshared ? 1 : nhs) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            if (offs) HIPCHK(hipMemcpyAsync(hin + 10 * nhs, h->mv.h, nhs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            if (rnd) {
                HIPCHK(hipMemcpyAsync(hin + 2 * nhs, rnd->eps_e, nhs * sizeof(double), hipMemcpyDeviceToHost, h->stream));
                HIPCHK(hipMemcpyAsync(hin + 3 * nhs, rnd->eps_t, nhs * h->d * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            }
            HIPCHK(hipStreamSynchronize(h->stream));
        }
        tgp_powers::plan_smooth_head_forward(mh, sp, yhead, mu_end, &quad_head, hhhead);
    }
    {
        LaunchScope ls(h, rnd ? "k_smooth_one<rand>" : (post ? "k_smooth_one<posterior>" : "k_smooth_one<logpdf>"));
        const int rc = tgp_powers::smooth_lti(h->stream, sp, overlap ? nullptr : mu_end, c);
        if (rc != 0) return h->fail(TGP_EHIP, std::string("tgp_posterior_marginals: launch: ") + hipGetErrorString((hipError_t)rc));
    }
    struct FlagGuard {      // (whatever path leaves from here on: no workgroup is left waiting for the host)
        long long* f;
        long long v;
        ~FlagGuard() {
            if (!f) return;
            for (int k : {1, 3})
                if (__atomic_load_n(f + k, __ATOMIC_RELAXED) < v) __atomic_store_n(f + k, v, __ATOMIC_RELEASE);
        }
    } guard{overlap ? sflag : nullptr, 2 * seq};
    auto await = [&](const long long* f) { return tgp_modal::await_host_flag(f, 2 * seq, h->stream); };
    bool handshake_ok = true;
    if (overlap) {
        if (hand) handshake_ok = await(sflag);
        if (handshake_ok) {
            tgp_powers::plan_smooth_head_forward(mh, sp, yhead, mu_end, &quad_head, hhhead);
            __atomic_store_n(sflag + 1, 2 * seq, __ATOMIC_RELEASE);
        }
    }
    const bool tables_ok = !post || tgp_powers::plan_smooth_head_tables(mh, sp);      // (beside the kernel)
    auto head_back = [&]() {
        if (rnd) {
            tgp_powers::plan_smooth_head_backward_rand(mh, sp, yhead, xi, eehead, ethead, rnhead, !rshared, hout);
            return;
        }
        tgp_powers::plan_smooth_head_backward(mh, sp, yhead, xi, hout, hout + nhs);
        for (size_t t = 0; t < nhs; ++t) hout[nhs + t] += rnhead[rshared ? 0 : t];
    };
    if (overlap && post && tables_ok && handshake_ok) {      // workgroup 0 is among the first to finish: its xi arrives long before the grid is through
        handshake_ok = await(sflag + 2);
        if (handshake_ok) {
            head_back();
            __atomic_store_n(sflag + 3, 2 * seq, __ATOMIC_RELEASE);
        }
    }
    tm.kernels_done();
    if (overlap) {
        for (int k : {1, 3})      // (a hand-over that failed, head tables that declined: no workgroup waits for what will not come; the outputs are discarded)
            if (__atomic_load_n(sflag + k, __ATOMIC_RELAXED) < 2 * seq) __atomic_store_n(sflag + k, 2 * seq, __ATOMIC_RELEASE);
        TRY(copy_back(h, mean_out, dm, nT, odev));
        TRY(copy_back(h, var_out, dv, nT, odev));
    }
    if (h->timing) (void)hipEventRecord(h->ev[3], h->stream);
    HIPCHK(hipStreamSynchronize(h->stream));
    resolve_profile(h);
    if (!handshake_ok) return h->fail(TGP_EHIP, "the one-launch smoother's host / device hand-over timed out");
    if (!tables_ok) {      // a head step's predicted covariance not positive definite: the older engines give the verdict
        h->smooth_state = -1;
        return TGP_OK;
    }
    if (!overlap) {
        if (post) {
            head_back();
            HIPCHK(hipMemcpyAsync(dm, hout, nhs * sizeof(double), hipMemcpyHostToDevice, h->stream));
            if (dv) HIPCHK(hipMemcpyAsync(dv, hout + nhs, nhs * sizeof(double), hipMemcpyHostToDevice, h->stream));
        }
        TRY(copy_back(h, mean_out, dm, nT, odev));
        TRY(copy_back(h, var_out, dv, nT, odev));
        HIPCHK(hipStreamSynchronize(h->stream));
    }
    double ssq = 0.0;
    for (long long g = 0; g < nwg; ++g) ssq += part[g];
    const double lml = head_lml(fp, h->T, quad_head, ssq);
    if (rnd && !(lml == lml)) return TGP_OK;      // (a NaN in the series -- NaN == missing in the mirrors' convention --: the evaluated route serves the draw)
    if (getenv("TGP_STEADY_DEBUG") != nullptr)
        fprintf(stderr, "[tgp smooth] T %lld post %d overlap %d idev %d odev %d nwg %lld nhs %d halo %d n1 %d seq %lld quad_head %.6g ssq %.6g lml %.10g\n", (long long)h->T,
                (int)post, (int)overlap, (int)idev, (int)odev, nwg, fp.nhs, sp.halo, sp.n1, seq, quad_head, ssq, lml);
    note_served(h, Served::dense, fp.n0, lml, lml_out);
    *served = true;
    return TGP_OK;
}

// rand of posterior(model, y) with replaced observation noise (lgssm.jl:65-91 on the reverse-time model of :193-221; posterior_lti_sde.jl:48-58)
// WITHOUT evaluating that model: Forward LTI models with scalar observations, one noise variance, no missing data, d <= 6 -- k_smooth_one with a
// noise input (DESIGN 3.17) --, or 8 < d <= 63 where the wide-state engine's plans accept the model -- its forward kernel and k_wide_post_rand (DESIGN 4.4).
// TGP_EUNSUPPORTED: the caller takes the evaluated route (tgp_posterior, then tgp_rand on the Reverse model).
int tgp_posterior_rand(tgp_handle* h, const double* y, const double* Rnew, const double* eps_t, const double* eps_e, const double* eps_0, uint32_t flags,
                       double* y_out) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (!y || !Rnew || !eps_t || !eps_e || !eps_0 || !y_out) return h->fail(TGP_EINVAL, "tgp_posterior_rand: null argument");
    bool served = false;
    const SmoothRand rnd{eps_t, eps_e, eps_0};
    if (steady2_eligible(h, nullptr, flags)) TRY(smooth_lti_call(h, y, flags, Rnew, y_out, nullptr, nullptr, &served, &rnd));
    if (!served && wide_eligible(h, y, nullptr)) TRY(wide_post_rand_call(h, y, flags, Rnew, eps_t, eps_e, eps_0, y_out, &served));
    if (!served)
        return h->fail(TGP_EUNSUPPORTED, "tgp_posterior_rand: Forward LTI models with scalar observations, one noise variance and d <= 6, or 8 < d <= 63 on the "
                                         "wide-state engine (take tgp_posterior + tgp_rand)");
    return TGP_OK;
}

// The same draw where the series has missing steps, the transitions or the noise are per step, or the observations are vectors with diagonal noise --
// what merge_datasets makes of rand(rng, posterior(fx, y)(x_new)) -- on the sweep engine's draw kernel (what sweep_eligible accepts: scalar observations,
// d <= 4, T >= 2048; DESIGN 4.7, k_sweep_draw) or on the dense engine's persistent passes (16 < d <= 64, p <= 16; DESIGN 4.6, tgp_dense_draw.hpp).
// TGP_EUNSUPPORTED: nothing was written to y_out, the caller takes the evaluated route.
int tgp_posterior_rand_missing(tgp_handle* h, const double* y, const uint8_t* missing, const double* Rnew, const double* eps_t, const double* eps_e,
                               const double* eps_0, uint32_t flags, double* y_out) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (!y || !Rnew || !eps_t || !eps_e || !eps_0 || !y_out) return h->fail(TGP_EINVAL, "tgp_posterior_rand_missing: null argument");
    if (sweep_eligible(h, flags)) {
        bool served = false;
        std::string why;
        TRY(sweep_draw_call(h, y, missing, flags, Rnew, eps_t, eps_e, eps_0, y_out, &served, &why));
        if (served) return TGP_OK;
        return h->fail(TGP_EUNSUPPORTED, "tgp_posterior_rand_missing: the sweep engine declines the draw: " + why + " (take tgp_posterior + tgp_rand)");
    }
    // (5 <= d <= 8 on the group sweep: tgp_posterior_rand_group, an entry point of its own -- this one declines there with no attempt made)
    if (!h->is_dense || h->ordering != 0 || h->d > 64 || h->p > 16 || !h->dense_fused || !h->dense_chunked)
        return h->fail(TGP_EUNSUPPORTED, "tgp_posterior_rand_missing: Forward models with scalar observations, d <= 4 and T >= 2048 on the sweep engine, or with "
                                         "16 < d <= 64 and p <= 16 on the dense engine's passes across the chip (else take tgp_posterior_rand, or "
                                         "tgp_posterior + tgp_rand)");
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0, rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * h->p * sizeof(double);
    CallTimer tm(h);
    const void *pR = nullptr, *pet = nullptr, *pee = nullptr;
    TRY(stage_in(h, h->bRnew, Rnew, rshared ? (size_t)h->p * sizeof(double) : nT, idev, &pR));
    TRY(set_obs(h, y, missing, flags & ~(uint32_t)TGP_REUSE_REDUCE));
    TRY(stage_in(h, h->beps_t, eps_t, (size_t)h->T * h->d * sizeof(double), idev, &pet));
    TRY(stage_in(h, h->beps_e, eps_e, nT, idev, &pee));
    tm.inputs_done();
    double* dy = nullptr;
    TRY(stage_out(h, h->bo1, y_out, nT, odev, &dy));
    tgp_dense::set_profile(h->dense, h->profile);
    TRY(dense_fail(h, tgp_dense::posterior_rand(h->dense, h->mv.y, h->mv.missing, (const double*)pR, rshared ? 0 : h->p, (const double*)pet, (const double*)pee,
                                                eps_0, h->mv.small_out, dy, h->result.d(), h->stream)));
    tm.kernels_done();
    TRY(copy_back(h, y_out, dy, nT, odev));
    return dense_finish(h, tm, nullptr);
}

// The same draw at state dimensions 5 .. 8 by the group sweep's draw kernel (k_sweep_group_draw, DESIGN 4.12): what sweep_group_eligible accepts, whatever
// the default routing of the engine's other calls (an explicit call; TGP_OPT_SWEEP >= 1).  tgp_posterior_rand_missing's arguments and flags.
int tgp_posterior_rand_group(tgp_handle* h, const double* y, const uint8_t* missing, const double* Rnew, const double* eps_t, const double* eps_e,
                             const double* eps_0, uint32_t flags, double* y_out) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (!y || !Rnew || !eps_t || !eps_e || !eps_0 || !y_out) return h->fail(TGP_EINVAL, "tgp_posterior_rand_group: null argument");
    if (!sweep_group_eligible(h, flags, /*post=*/true, /*explicit_call=*/true))
        return h->fail(TGP_EUNSUPPORTED, "tgp_posterior_rand_group: Forward models with shared A, a, Q, H (not SDE-described), scalar observations, 5 <= d <= 8 "
                                         "and T >= 2048 on the group sweep (TGP_OPT_SWEEP >= 1, the engine not declined for the bound model); use "
                                         "tgp_posterior_rand_missing at d <= 4 and tgp_posterior + tgp_rand otherwise");
    bool served = false;
    std::string why;
    TRY(sweep_group_draw_call(h, y, missing, flags, Rnew, eps_t, eps_e, eps_0, y_out, &served, &why));
    if (served) return TGP_OK;
    return h->fail(TGP_EUNSUPPORTED, "tgp_posterior_rand_group: the group sweep declines the draw: " + why + " (take tgp_posterior + tgp_rand)");
}

// logpdf and its gradient with respect to the shared blocks, and to the noise variance and the emission offset of every step, where the gains vary in time
// -- missing steps, a noise variance or an emission offset per step -- by ONE adjoint pass on the sweep engine (k_sweep_adjoint, DESIGN 4.8): what
// sweep_eligible accepts in LTI form.  TGP_EUNSUPPORTED: no output was written, the caller takes tgp_logpdf_grad.
int tgp_logpdf_adjoint_missing(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, double* lml_out, double* gA, double* ga, double* gQ,
                               double* gH, double* ghh, double* gR, double* gx0m, double* gx0P, double* gh_steps, double* gR_steps) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (!y) return h->fail(TGP_EINVAL, "tgp_logpdf_adjoint_missing: null argument");
    if (h->sde || !sweep_eligible(h, flags))
        return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint_missing: Forward models with shared A, a, Q, H (not SDE-described), scalar observations, d <= 4 and "
                                         "T >= 2048 on the sweep engine (TGP_OPT_SWEEP = 1, the engine not declined for the bound model); use tgp_logpdf_grad "
                                         "otherwise");
    tgp_sweep::AdjointOut o;
    o.gA = gA; o.ga = ga; o.gQ = gQ; o.gH = gH; o.ghh = ghh; o.gR = gR; o.gx0m = gx0m; o.gx0P = gx0P;
    bool served = false;
    std::string why;
    TRY(sweep_adjoint_call(h, y, missing, flags, lml_out, o, gh_steps, gR_steps, &served, &why));
    if (served) return TGP_OK;
    return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint_missing: the sweep engine declines the gradient: " + why + " (use tgp_logpdf_grad)");
}

// The same at state dimensions 5 .. 8 by the group sweep's adjoint kernel (k_sweep_group_adjoint, DESIGN 4.11): what sweep_group_eligible accepts, whatever
// the default routing of the engine's other calls (an explicit call; TGP_OPT_SWEEP >= 1).  tgp_logpdf_adjoint_missing's arguments and outputs.
int tgp_logpdf_adjoint_group(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, double* lml_out, double* gA, double* ga, double* gQ,
                             double* gH, double* ghh, double* gR, double* gx0m, double* gx0P, double* gh_steps, double* gR_steps) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (!y) return h->fail(TGP_EINVAL, "tgp_logpdf_adjoint_group: null argument");
    if (!sweep_group_eligible(h, flags, /*post=*/true, /*explicit_call=*/true))
        return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint_group: Forward models with shared A, a, Q, H (not SDE-described), scalar observations, 5 <= d <= 8 "
                                         "and T >= 2048 on the group sweep (TGP_OPT_SWEEP >= 1, the engine not declined for the bound model); use "
                                         "tgp_logpdf_adjoint_missing at d <= 4 and tgp_logpdf_grad otherwise");
    tgp_sweep::AdjointOut o;
    o.gA = gA; o.ga = ga; o.gQ = gQ; o.gH = gH; o.ghh = ghh; o.gR = gR; o.gx0m = gx0m; o.gx0P = gx0P;
    bool served = false;
    std::string why;
    TRY(sweep_group_adjoint_call(h, y, missing, flags, lml_out, o, gh_steps, gR_steps, &served, &why));
    if (served) return TGP_OK;
    return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint_group: the group sweep declines the gradient: " + why + " (use tgp_logpdf_grad)");
}

// The same for a model described by its SDE and time stamps (tgp_model_set_sde: irregular spacing) -- what sweep_eligible accepts in SDE form -- by the
// engine's k_sweep_adjoint_sde (DESIGN 4.9).  The kernel leaves the sums over the closed form's coefficients (lam, N1, N2), Pinf and the explicit first
// transition; the host finishes d logpdf / d F by the transpose of sde_closed_form's map.  A model bound without A1 takes exp(F 1) at step 0
// (tgp_model_set_sde): that step's G_0 is contracted into the coefficient sums with tau = 1 and gA1 is zero.
int tgp_logpdf_adjoint_sde(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, double* lml_out, double* gF, double* gPinf, double* gA1,
                           double* ga, double* gH, double* ghh, double* gR, double* gx0m, double* gx0P, double* gh_steps, double* gR_steps) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (!y) return h->fail(TGP_EINVAL, "tgp_logpdf_adjoint_sde: null argument");
    if (!h->sde)
        return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint_sde: the model is not SDE-described (tgp_model_set_sde); use tgp_logpdf_adjoint_missing for models in "
                                         "LTI form");
    if (!sweep_eligible(h, flags))
        return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint_sde: Forward SDE-described models with closed-form transitions (TGP_OPT_SDE_CLOSED_FORM = 1), shared a "
                                         "and H, scalar observations, d <= 4 and T >= 2048 on the sweep engine (TGP_OPT_SWEEP = 1, the engine not declined for the "
                                         "bound model); use tgp_logpdf_grad_sde otherwise");
    const int d = h->d, dd = d * d;
    double buf[4 * 16 + 3 * 4 + 2 + 2 * 16];
    tgp_sweep::AdjointSdeOut so;
    so.gl = buf; so.gN1 = so.gl + d; so.gN2 = so.gN1 + dd; so.gPinf = so.gN2 + dd; so.gA1 = so.gPinf + dd; so.ga = so.gA1 + dd; so.gH = so.ga + d;
    so.ghh = so.gH + d; so.gR = so.ghh + 1; so.gx0m = so.gR + 1; so.gx0P = so.gx0m + d;
    bool served = false;
    std::string why;
    TRY(sweep_adjoint_call(h, y, missing, flags, lml_out, tgp_sweep::AdjointOut(), gh_steps, gR_steps, &served, &why, &so));
    if (!served) return h->fail(TGP_EUNSUPPORTED, "tgp_logpdf_adjoint_sde: the sweep engine declines the gradient: " + why + " (use tgp_logpdf_grad_sde)");
    const double* coef = h->sde_coef_host.data();
    if (!h->have_AQ1) {      // step 0 took A1 = E (I + N1 + N2), E = diag(e^(-lam_i)): its G_0 belongs to the coefficients
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
    if (gF) sde_coef_to_gF(d, coef, so.gl, so.gN1, so.gN2, gF);
    if (gPinf) std::memcpy(gPinf, so.gPinf, sizeof(double) * dd);
    if (gA1) std::memcpy(gA1, so.gA1, sizeof(double) * dd);
    if (ga) std::memcpy(ga, so.ga, sizeof(double) * d);
    if (gH) std::memcpy(gH, so.gH, sizeof(double) * d);
    if (ghh) *ghh = *so.ghh;
    if (gR) *gR = *so.gR;
    if (gx0m) std::memcpy(gx0m, so.gx0m, sizeof(double) * d);
    if (gx0P) std::memcpy(gx0P, so.gx0P, sizeof(double) * dd);
    return TGP_OK;
}

// Two observations per step of ONE latent value with independent noise are one observation of it:
//     N(y; f, R) N(y*; f, R*) = N(ybar; f, Rbar) N(y - y*; 0, R + R*),   Rbar = R R* / (R + R*),   ybar = (R* y + R y*) / (R + R*)
// -- what turns logpdf(replace_observation_noise_cov(posterior(model, y), R*), y*) (posterior_lti_sde.jl:62-78 -> lgssm.jl:147-151 on the
// reverse-time model of lgssm.jl:193-221) into two logpdf calls of the PRIOR: logpdf(model(Rbar), ybar) + pair - logpdf(model(R), y), DESIGN 3.18.
// One pass over the two series: 16 bytes read and 8 written per step (+ 8 per per-step variance read or written, + the masks).
namespace {
struct PairArgs {
    const double *y, *R, *ys, *Rs;
    const uint8_t *m, *ms;
    double *ybar, *Rbar, *part;
    uint8_t* mbar;
    long long n;
    double R0, Rs0;
};
static __global__ __launch_bounds__(256) void k_pair_statistic(const PairArgs a) {
    const long long stride = (long long)gridDim.x * 256;
    const double tot0 = a.R0 + a.Rs0, lg0 = log(6.283185307179586 * tot0);
    double acc = 0.0;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < a.n; i += stride) {
        const double y = a.y[i], ys = a.ys[i];
        const double R = a.R ? a.R[i] : a.R0, Rs = a.Rs ? a.Rs[i] : a.Rs0;
        const bool my = a.m && a.m[i] != 0, mn = a.ms && a.ms[i] != 0;
        double yb, Rb;
        if (!my && !mn) {
            const double tot = R + Rs, df = y - ys;
            acc -= 0.5 * (((a.R || a.Rs) ? log(6.283185307179586 * tot) : lg0) + df * df / tot);
            yb = (Rs * y + R * ys) / tot;       // (no division by a jitter-sized R*)
            Rb = R * Rs / tot;
        } else if (!my) {
            yb = y, Rb = R;
        } else if (!mn) {
            yb = ys, Rb = Rs;
        } else {
            yb = 0.0, Rb = R;                   // missing on both sides: the joint step is missing
        }
        a.ybar[i] = yb;
        if (a.Rbar) a.Rbar[i] = Rb;
        if (a.mbar) a.mbar[i] = (my && mn) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    __shared__ double sw[4];
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) a.part[blockIdx.x] = (sw[0] + sw[1]) + (sw[2] + sw[3]);
}
}  // namespace

int tgp_pair_statistic(tgp_handle* h, int64_t n, const double* y, const uint8_t* missing, const double* R, int64_t nR, const double* y_new,
                       const uint8_t* missing_new, const double* R_new, int64_t nR_new, double* ybar, double* Rbar, uint8_t* missing_bar,
                       double* pair_out) {
    if (!h) return TGP_EINVAL;
    if (n < 0 || !y || !y_new || !R || !R_new || !ybar || !pair_out || (nR != 1 && nR != n) || (nR_new != 1 && nR_new != n))
        return h->fail(TGP_EINVAL, "tgp_pair_statistic: null argument, or a variance count that is neither 1 nor n");
    const bool per_step = nR == n && n > 1, per_step_new = nR_new == n && n > 1;
    if (!Rbar && (per_step || per_step_new || missing || missing_new))
        return h->fail(TGP_EINVAL, "tgp_pair_statistic: Rbar [n] is needed when a variance is per step or anything is missing");
    if (!missing_bar && missing && missing_new) return h->fail(TGP_EINVAL, "tgp_pair_statistic: missing_bar [n] is needed with two masks");
    *pair_out = 0.0;
    if (n == 0) return TGP_OK;
    TRY(bind_device(h));
    PairArgs a{};
    a.y = y, a.ys = y_new, a.m = missing, a.ms = missing_new, a.ybar = ybar, a.Rbar = Rbar, a.mbar = (missing && missing_new) ? missing_bar : nullptr, a.n = n;
    a.R = per_step ? R : nullptr;
    a.Rs = per_step_new ? R_new : nullptr;
    a.R0 = a.Rs0 = 1.0;
    // (a single variance is read on the host: a device value when n == 1 says both are per step -- one 8-byte copy each)
    if (!per_step) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, R) == hipSuccess && at.type == hipMemoryTypeDevice) HIPCHK(hipMemcpy(&a.R0, R, sizeof(double), hipMemcpyDeviceToHost));
        else { (void)hipGetLastError(); a.R0 = R[0]; }
    }
    if (!per_step_new) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, R_new) == hipSuccess && at.type == hipMemoryTypeDevice) HIPCHK(hipMemcpy(&a.Rs0, R_new, sizeof(double), hipMemcpyDeviceToHost));
        else { (void)hipGetLastError(); a.Rs0 = R_new[0]; }
    }
    if (!(a.R0 + a.Rs0 > 0.0)) return h->fail(TGP_EINVAL, "tgp_pair_statistic: R + R_new must be positive");
    const int nblk = (int)std::min<long long>(2048, (n + 1023) / 1024);
    TRY(ensure_pinned(h, (size_t)nblk));
    a.part = h->flt_host;
    hipLaunchKernelGGL(k_pair_statistic, dim3(nblk), dim3(256), 0, h->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(h->stream));
    double sum = 0.0;
    for (int b = 0; b < nblk; ++b) sum += h->flt_host[b];
    *pair_out = sum;
    return TGP_OK;
}

