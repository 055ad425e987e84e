// Part of tgp_api.hip (included there, one translation unit): time segments on the one-launch path, the plan and adjoint entry points without a handle.
// ---- time segments on the one-launch path (one rank of several; tgp_multi.hip and the one-process-per-GPU driver) ----------------------
// Both mean recursions forget a state within `halo` steps, so a rank needs nothing of its neighbours but their `halo` observations next to
// the boundary: no exchange of filter elements, no carry between ranks.  The plan is a function of the model blocks and the series' length
// only -- every rank computes the same one, and the same verdict for every segment.
static bool modal_host_model(tgp_handle* h, tgp_plan::ModelHost& mh) {
    if (!h->opt_modal || h->hostm.empty()) return false;
    const int d = h->d;
    const size_t dd = (size_t)d * d;
    const double* q = h->hostm.data();
    mh.d = d;
    mh.A = q; mh.a = q + dd; mh.Q = q + dd + d; mh.H = q + 2 * dd + d; mh.hh = q + 2 * dd + 2 * d; mh.R = h->has_R_over ? &h->R_over : q + 2 * dd + 2 * d + 1;
    mh.x0m = h->x0m.data();
    mh.x0P = h->x0P.data();
    return true;
}

int tgp_segment_plan(tgp_handle* h, int64_t T_total, int nseg, const int64_t* bounds, int32_t* applies, int32_t* halo) {
    if (!h || !bounds || !applies || !halo || nseg < 1 || T_total <= 0) return TGP_EINVAL;
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    *applies = 0;
    *halo = 0;
    tgp_plan::ModelHost mh;
    if (!modal_host_model(h, mh) || h->ordering != 0 || h->p != 1 || h->sde) return TGP_OK;
    if (bounds[0] != 0 || bounds[nseg] != T_total) return h->fail(TGP_EINVAL, "tgp_segment_plan: the segments must tile [0, T)");
    if (!h->modal) h->modal = tgp_modal::create();
    if (!tgp_modal::plan(h->modal, mh, T_total)) return TGP_OK;
    ModalFlagGuard flag_guard{h->modal};
    (void)tgp_modal::complete(h->modal, T_total);      // (the verdict of the tables half is part of the answer: every rank must give the same one)
    if (tgp_modal::last_plan(h->modal).why != 0) return TGP_OK;
    const tgp_plan::Modal& md = tgp_modal::last_modal(h->modal);
    bool ok = true;
    for (int r = 0; r < nseg && ok; ++r) {
        const int64_t lo = bounds[r], hi = bounds[r + 1];
        ok = hi > lo && lo % 16 == 0 && (hi % 16 == 0 || hi == T_total) && hi - lo >= md.halo;
        if (r > 0) ok = ok && lo >= (int64_t)md.nhs + md.halo;
        if (r == 0) ok = ok && hi >= (int64_t)md.nhs + 16;
        if (r == nseg - 1) ok = ok && hi - lo >= md.n1 + 16;
    }
    *applies = ok ? 1 : 0;
    *halo = md.halo;
    return TGP_OK;
}

int tgp_segment_logpdf_and_posterior_marginals(tgp_handle* h, int64_t T_total, int64_t seg_lo, int64_t seg_hi, const double* y_seg, const double* y_left,
                                               const double* y_right, const double* Rnew, uint32_t flags, double* mean_out, double* var_out,
                                               double* lml_share) {
    if (!h || !lml_share) return TGP_EINVAL;
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    tgp_plan::ModelHost mh;
    if (!modal_host_model(h, mh)) return h->fail(TGP_EUNSUPPORTED, "tgp_segment_*: not a model of the one-launch path (ask tgp_segment_plan first)");
    if (h->T != seg_hi - seg_lo || seg_lo < 0 || seg_hi > T_total || !y_seg) return h->fail(TGP_EINVAL, "tgp_segment_*: the bound model has not the segment's length");
    if ((mean_out != nullptr) != (var_out != nullptr) || (mean_out && !Rnew)) return h->fail(TGP_EINVAL, "tgp_segment_*: mean, var and Rnew go together");
    if (!h->modal) h->modal = tgp_modal::create();
    if (!tgp_modal::plan(h->modal, mh, T_total)) return h->fail(TGP_EUNSUPPORTED, "tgp_segment_*: the one-launch path does not apply to this model / series");
    const tgp_plan::Modal& md = tgp_modal::last_modal(h->modal);
    if ((seg_lo > 0 && !y_left) || (seg_hi < T_total && !y_right)) return h->fail(TGP_EINVAL, "tgp_segment_*: the neighbours' observations are missing");
    {   // the per-segment conditions of tgp_segment_plan, again: a direct caller with other bounds gets an error, not wrong numbers (round-4 advice)
        bool ok = seg_lo % 16 == 0 && (seg_hi % 16 == 0 || seg_hi == T_total) && seg_hi - seg_lo >= md.halo;
        if (seg_lo > 0) ok = ok && seg_lo >= (int64_t)md.nhs + md.halo;
        else ok = ok && seg_hi >= (int64_t)md.nhs + 16;
        if (!ok) return h->fail(TGP_EUNSUPPORTED, "tgp_segment_*: bounds the one-launch path does not serve (multiples of 16, a segment holds the halo, the first one the head: tgp_segment_plan)");
    }
    const bool odev = (flags & TGP_OUT_DEVICE) != 0, rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    CallTimer tm(h, /*clear=*/false);
    const void* pR = nullptr;
    if (mean_out) TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, (flags & TGP_IN_DEVICE) != 0, &pR));
    obs_changed(h);
    h->mv.y = y_seg;
    h->mv.missing = nullptr;
    tm.inputs_done();
    double *dm = nullptr, *dv = nullptr;
    TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
    TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
    tgp_modal::Call c;
    c.T = T_total;
    c.y = y_seg;
    c.Rnew = static_cast<const double*>(pR);
    c.rnew_per_step = (mean_out && !rshared) ? 1 : 0;
    c.mean = dm;
    c.var = dv;
    c.seg_lo = seg_lo;
    c.seg_hi = seg_hi;
    c.yl = y_left;
    c.yr = y_right;
    {
        std::string err;
        const char* kname = tgp_modal::kernel_name(h->modal, dm != nullptr);
        LaunchScope ls(h, kname);
        if (tgp_modal::enqueue(h->modal, h->stream, c, &kname, &err) != 0) return h->fail(TGP_EHIP, err);
    }
    ModalFlagGuard flag_guard{h->modal};
    const bool tables_ok = tgp_modal::complete(h->modal, T_total);
    tm.kernels_done();
    TRY(copy_back(h, mean_out, dm, nT, odev));
    TRY(copy_back(h, var_out, dv, nT, odev));
    HIPCHK(hipStreamSynchronize(h->stream));
    resolve_profile(h);
    if (!tables_ok) return h->fail(TGP_EUNSUPPORTED, "tgp_segment_*: the plan's tables half declined (tgp_segment_plan would have said so)");
    double ssq = 0.0, hq = 0.0;
    tgp_modal::finish_parts(h->modal, &ssq, &hq);
    double share = -0.5 * (hq + md.iS * ssq);
    if (seg_lo == 0) share += head_lml(md, T_total, 0.0, 0.0);      // (the head's and the stationary steps' constant terms: the first segment's)
    note_served(h, Served::modal, tgp_modal::last_plan(h->modal).n0, share, lml_share);
    return TGP_OK;
}

// Host-only (no GPU needed): the plan the one-launch path of the stationary-gain engine builds inside every call (tgp_steady_plan.hpp).
int tgp_steady_plan(int d, const double* A, const double* a, const double* Q, const double* H, const double* hh, const double* R, const double* x0m,
                    const double* x0P, int64_t T, int32_t* info_i, double* info_d, double* modal_out, double* tables_out) {
    if (d < 1 || d > tgp_plan::kMaxD || !A || !a || !Q || !H || !hh || !R || !x0m || !x0P || T <= 0 || !info_i || !info_d) return TGP_EINVAL;
    static thread_local tgp_plan::HeadTables tab;
    tgp_plan::Modal md{};
    tgp_plan::ModelHost mh;
    mh.d = d;
    mh.A = A; mh.a = a; mh.Q = Q; mh.H = H; mh.hh = hh; mh.R = R; mh.x0m = x0m; mh.x0P = x0P;
    const tgp_plan::Info in = tgp_modal::plan_only(mh, T, md, tab);
    info_i[0] = in.why; info_i[1] = in.n0; info_i[2] = in.n1; info_i[3] = in.why == 0 ? md.nhs : 0; info_i[4] = in.halo; info_i[5] = in.why == 0 ? md.npair : 0;
    {
        int nw = 8, sub = 8;
        tgp_modal::choose_geometry(d, in.halo, &nw, &sub);
        info_i[6] = nw;
        info_i[7] = sub;
    }
    info_d[0] = in.cond_f; info_d[1] = in.cond_g; info_d[2] = in.rho; info_d[3] = in.resid;
    if (in.why != 0) return TGP_OK;
    if (modal_out) {
        double* q = modal_out;
        const double* arrs[17] = {md.fd, md.fo, md.fb, md.fa, md.fw, md.gd, md.go, md.gc, md.gw, md.fp8r, md.fp8i, md.gp8r, md.gp8i, md.fp512r, md.fp512i, md.gp512r, md.gp512i};
        for (const double* ar : arrs)
            for (int i = 0; i < tgp_plan::kMaxD; ++i) *q++ = ar[i];
        for (int j = 0; j < tgp_plan::kSub; ++j)
            for (int i = 0; i < tgp_plan::kMaxD; ++i) *q++ = md.WJ[j][i];
        for (int j = 0; j < tgp_plan::kSub; ++j)
            for (int i = 0; i < tgp_plan::kMaxD; ++i) *q++ = md.WG[j][i];
        *q++ = md.hh; *q++ = md.rS; *q++ = md.iS; *q++ = md.logS; *q++ = md.LS; *q++ = md.vb;
    }
    if (tables_out) {
        double* q = tables_out;
        const int n = md.n0 + 1, dd = d * d;
        for (int i = 0; i < tgp_plan::kMaxD; ++i) *q++ = tab.h[i];
        for (int i = 0; i < tgp_plan::kMaxD; ++i) *q++ = tab.mu0[i];
        for (int i = 0; i < tgp_plan::kMaxD * tgp_plan::kMaxD; ++i) *q++ = tab.Wm[i];
        for (int i = 0; i < n * d; ++i) *q++ = tab.kA[i];
        for (int i = 0; i < n; ++i) *q++ = tab.iS[i];
        for (int i = 0; i < n; ++i) *q++ = tab.rS[i];
        for (int i = 0; i < n * dd; ++i) *q++ = tab.G[i];
        for (int i = 0; i < n * d; ++i) *q++ = tab.c[i];
        for (int i = 0; i < n; ++i) *q++ = tab.vb[i];
        for (int i = 0; i < md.n1; ++i) *q++ = tab.tvb[i];
    }
    return TGP_OK;
}

// Host-only (no GPU needed): the FILTER plan (tgp_plan::FilterPlan through tgp_powers::plan_filter) that k_adjoint_one, k_filter_one and the dense-powers
// smoother are laid out on -- head length and halo decide where their spans, tiles and workgroups begin and end (tests place their lengths by it).
int tgp_filter_plan(int d, const double* A, const double* a, const double* Q, const double* H, const double* hh, const double* R, const double* x0m,
                    const double* x0P, int64_t T, int32_t* info) {
    if (d < 1 || d > tgp_plan::kRandMaxD || !A || !a || !Q || !H || !hh || !R || !x0m || !x0P || T <= 0 || !info) return TGP_EINVAL;
    tgp_plan::ModelHost mh;
    mh.d = d;
    mh.A = A; mh.a = a; mh.Q = Q; mh.H = H; mh.hh = hh; mh.R = R; mh.x0m = x0m; mh.x0P = x0P;
    tgp_plan::FilterPlan fp;
    tgp_powers::plan_filter(mh, T, fp);
    info[0] = fp.why; info[1] = fp.n0; info[2] = fp.nhs; info[3] = fp.halo;
    return TGP_OK;
}

// Host-only (no GPU needed): the plan of the dense-powers smoother (tgp_plan::SmoothPlan through tgp_powers::plan_smooth, the very call smooth_lti_call
// makes) -- k_smooth_one<logpdf> with want_posterior == 0, k_smooth_one<posterior> and k_smooth_one<rand> otherwise.  span and workgroups are
// tgp_powers::smooth_span / smooth_workgroups; both stay 0 where the plan stopped before its halo was known, workgroups also where it declined.
int tgp_smooth_plan(int d, const double* A, const double* a, const double* Q, const double* H, const double* hh, const double* R, const double* x0m,
                    const double* x0P, int64_t T, int want_posterior, int32_t* info) {
    if (d < 1 || d > tgp_plan::kRandMaxD || !A || !a || !Q || !H || !hh || !R || !x0m || !x0P || T <= 0 || !info) return TGP_EINVAL;
    tgp_plan::ModelHost mh;
    mh.d = d;
    mh.A = A; mh.a = a; mh.Q = Q; mh.H = H; mh.hh = hh; mh.R = R; mh.x0m = x0m; mh.x0P = x0P;
    static thread_local tgp_plan::SmoothPlan sp;
    static thread_local double tvb[tgp_plan::kTailMax];
    const bool post = want_posterior != 0;
    sp = tgp_plan::SmoothPlan{};
    tgp_powers::plan_smooth(mh, T, sp, tvb, post);
    info[0] = sp.why; info[1] = sp.fp.n0; info[2] = sp.fp.nhs; info[3] = sp.fp.halo; info[4] = sp.halo; info[5] = sp.n1;
    info[6] = sp.halo > 0 ? (int32_t)tgp_powers::smooth_span(sp, post) : 0;
    info[7] = sp.why == tgp_plan::kOk ? (int32_t)tgp_powers::smooth_workgroups(sp, T, post) : 0;
    return TGP_OK;
}

// Host-only (no GPU needed): the plan k_rand_one is launched on (tgp_plan::RandPlan through tgp_powers::plan_rand: a function of the model alone; tgp_rand
// takes the path when why == 0 and T >= 2).  span = tgp_powers::rand_span, workgroups = ceil(T / span): there is no head, the first workgroup starts at step 0.
int tgp_rand_plan(int d, const double* A, const double* a, const double* Q, const double* H, const double* hh, const double* R, const double* x0m,
                  const double* x0P, int64_t T, int32_t* info) {
    if (d < 1 || d > tgp_plan::kRandMaxD || !A || !a || !Q || !H || !hh || !R || !x0m || !x0P || T <= 0 || !info) return TGP_EINVAL;
    tgp_plan::ModelHost mh;
    mh.d = d;
    mh.A = A; mh.a = a; mh.Q = Q; mh.H = H; mh.hh = hh; mh.R = R; mh.x0m = x0m; mh.x0P = x0P;
    static thread_local tgp_plan::RandPlan rp;
    rp = tgp_plan::RandPlan{};
    tgp_powers::plan_rand(mh, rp);
    const bool ok = rp.why == tgp_plan::kOk;
    info[0] = rp.why; info[1] = rp.halo;
    info[2] = ok ? (int32_t)tgp_powers::rand_span(rp) : 0;
    info[3] = ok ? (int32_t)tgp_powers::rand_workgroups(rp, T) : 0;
    return TGP_OK;
}

// The host plan of the wide-state engine (tgp_wide.hip) without a handle or a GPU (the CPU tier checks it against the discrete Riccati equation).
int tgp_wide_plan(int d, const double* A, const double* a, const double* Q, const double* H, const double* hh, const double* R, const double* x0m, const double* x0P, int64_t T,
                  int want_posterior, int64_t* info, double* Kss, double* Sss, double* var_parts) {
    if (!tgp_wide::supports(d) || !A || !a || !Q || !H || !hh || !R || !x0m || !x0P || !info) return TGP_EINVAL;
    tgp_wide::Engine* e = tgp_wide::create();
    tgp_wide::ModelHost m;
    m.d = d;
    m.A = A; m.a = a; m.Q = Q; m.H = H; m.hh = *hh; m.R = *R; m.x0m = x0m; m.x0P = x0P;
    const bool ok = tgp_wide::plan(e, m, T);
    const bool okp = ok && want_posterior && tgp_wide::plan_posterior(e, T);
    const tgp_wide::Info& in = tgp_wide::last_plan(e);
    info[0] = in.why; info[1] = in.n0; info[2] = in.halo; info[3] = want_posterior ? in.why_post : -1; info[4] = in.n1; info[5] = in.halo_back;
    info[6] = in.chunks; info[7] = in.chunk_len;
    if (ok) {
        double vb = 0.0, qi = 0.0;
        tgp_wide::stationary(e, Kss, Sss, &vb, &qi);
        if (var_parts && okp) { var_parts[0] = vb; var_parts[1] = qi; }
    }
    tgp_wide::destroy(e);
    return TGP_OK;
}

// ... and its draw half (tgp_wide::plan_draw: the reverse-time transition of lgssm.jl:231-238 at the settled filter covariance), likewise without a handle or a GPU.
int tgp_wide_plan_draw(int d, const double* A, const double* a, const double* Q, const double* H, const double* hh, const double* R, const double* x0m, const double* x0P,
                       int64_t T, int64_t* info, double* G, double* L, double* U) {
    if (!tgp_wide::supports(d) || !A || !a || !Q || !H || !hh || !R || !x0m || !x0P || !info) return TGP_EINVAL;
    tgp_wide::Engine* e = tgp_wide::create();
    tgp_wide::ModelHost m;
    m.d = d;
    m.A = A; m.a = a; m.Q = Q; m.H = H; m.hh = *hh; m.R = *R; m.x0m = x0m; m.x0P = x0P;
    const bool ok = tgp_wide::plan(e, m, T);
    const bool okd = ok && tgp_wide::plan_draw(e, T);
    const tgp_wide::Info& in = tgp_wide::last_plan(e);
    info[0] = in.why; info[1] = in.n0; info[2] = ok ? in.why_draw : -1; info[3] = in.halo_draw; info[4] = in.draw_chunks; info[5] = in.draw_chunk_len;
    if (okd) tgp_wide::draw_stationary(e, G, L, U);
    tgp_wide::destroy(e);
    return TGP_OK;
}

int tgp_adjoint_record_size(int d) { return (d >= 1 && d <= tgp_steady::kMaxD) ? tgp_adjoint::record_size(d) : 0; }

int tgp_adjoint_finish(int d, const double* rec, const double* y_head, int64_t n_head, double* gA, double* ga, double* gQ, double* gH,
                       double* ghh, double* gR, double* gx0m, double* gx0P) {
    if (d < 1 || d > tgp_steady::kMaxD || !rec || !y_head) return TGP_EINVAL;
    const tgp_adjoint::Out o{gA, ga, gQ, gH, ghh, gR, gx0m, gx0P};
    return tgp_adjoint::finish(d, rec, y_head, n_head, o) == 0 ? TGP_OK : TGP_EINVAL;
}

int tgp_adjoint_finish_wide(int d, const double* rec, int64_t rec_len, const double* y_head, int64_t n_head, int64_t head_steps, double* gA, double* ga, double* gQ,
                            double* gH, double* ghh, double* gR, double* gx0m, double* gx0P) {
    if (d < 1 || d > tgp_wide::kMaxD || !rec || !y_head || rec_len != tgp_adjoint::record_size(d)) return TGP_EINVAL;
    const tgp_adjoint::Out o{gA, ga, gQ, gH, ghh, gR, gx0m, gx0P};
    const int rc = tgp_wide::adjoint_finish_host(d, rec, y_head, n_head, head_steps, o);
    return rc == 0 ? TGP_OK : (rc < 0 ? TGP_EUNSUPPORTED : TGP_EINVAL);
}

// the pinned host buffer of the head-on-the-host paths (head observations in, head outputs and the workgroups' partial sums out)
