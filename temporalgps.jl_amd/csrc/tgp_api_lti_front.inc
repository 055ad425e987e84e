// Part of tgp_api.hip (included there, one translation unit): Reverse-ordered LTI priors by flipping the series, wide LTI models (tgp_wide.hip), logpdf of an LTI model on the one-launch kernels.
static int filter_lti_call(tgp_handle* h, const double* y, uint32_t flags, double* m_out, double* P_out, double* lml_out, bool* served);
struct SmoothRand {      // a draw from the posterior instead of its marginals: eps_t [T][d], eps_e [T] (where TGP_IN_DEVICE says), eps_0 [d] (host)
    const double *eps_t, *eps_e, *eps_0;
};
static int smooth_lti_call(tgp_handle* h, const double* y, uint32_t flags, const double* Rnew, double* mean_out, double* var_out, double* lml_out, bool* served,
                           const SmoothRand* rnd = nullptr);
static bool lti_but_offset(const tgp_handle* h);

// ---- Reverse-ordered LTI priors (lgssm.jl:87-91, 111-115, 161-165): with every block shared and x0 stationary, the Reverse model on y IS the
// Forward model on the flipped series (oracle identity: tests/test_oracle_identities.py) -- one flip pass in front of the one-launch kernels (and one behind them for
// outputs of size T) instead of the general chunked scan.
namespace {
__global__ __launch_bounds__(256) void k_flip_rows(const double* __restrict__ in, double* __restrict__ out, long long T, int w) {
    const long long n = T * w;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long t = i / w, c = i - t * w;
        out[i] = in[(T - 1 - t) * w + c];
    }
}
void launch_flip(tgp_handle* h, const double* in, double* out, long long T, int w) {
    const long long n = T * w;
    const unsigned nb = (unsigned)std::min<long long>((n + 255) / 256, 8192);
    LaunchScope ls(h, "k_flip_rows");
    hipLaunchKernelGGL(k_flip_rows, dim3(nb), dim3(256), 0, h->stream, in, out, T, w);
}
struct AsForward {      // the handle as its Forward twin for the length of a call
    tgp_handle* h;
    int o, mo;
    explicit AsForward(tgp_handle* h_) : h(h_), o(h_->ordering), mo(h_->mv.ordering) {
        h->ordering = 0;
        h->mv.ordering = 0;
    }
    ~AsForward() {
        h->ordering = o;
        h->mv.ordering = mo;
    }
};
// x0 = its own one-step prediction (A x0.m + a = x0.m, A x0.P A' + Q = x0.P to rounding): what to_sde's models have (x0 = the stationary distribution).
// A Reverse-ordered model updates with y_T BEFORE its first prediction, the Forward one predicts first: the two agree on flipped series only then.
bool x0_is_stationary(const tgp_handle* h) {
    const int d = h->d;
    const size_t dd = (size_t)d * d;
    if (h->hostm.size() < 2 * dd + d || h->x0m.size() != (size_t)d || h->x0P.size() != dd) return false;
    const double *A = h->hostm.data(), *a = A + dd, *Q = a + d;      // column-major blocks
    const double *m = h->x0m.data(), *P = h->x0P.data();
    double mmax = 0.0, pmax = 0.0;
    for (int i = 0; i < d; ++i) mmax = std::max(mmax, std::fabs(m[i]));
    for (size_t i = 0; i < dd; ++i) pmax = std::max(pmax, std::fabs(P[i]));
    std::vector<double> AP(dd, 0.0);
    for (int i = 0; i < d; ++i) {
        double v = a[i];
        for (int k = 0; k < d; ++k) v += A[i + (size_t)k * d] * m[k];
        if (!(std::fabs(v - m[i]) <= 1e-13 * (1.0 + mmax))) return false;
        for (int j = 0; j < d; ++j) {
            double w = 0.0;
            for (int k = 0; k < d; ++k) w += A[i + (size_t)k * d] * 0.5 * (P[k + (size_t)j * d] + P[j + (size_t)k * d]);
            AP[i + (size_t)j * d] = w;
        }
    }
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            double v = 0.5 * (Q[i + (size_t)j * d] + Q[j + (size_t)i * d]);
            for (int k = 0; k < d; ++k) v += AP[i + (size_t)k * d] * A[j + (size_t)k * d];
            if (!(std::fabs(v - 0.5 * (P[i + (size_t)j * d] + P[j + (size_t)i * d])) <= 1e-13 * pmax)) return false;
        }
    return true;
}
bool reverse_by_flip(const tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags) {
    static const bool on = [] {      // TGP_REVERSE_FLIP=0: Reverse-ordered models on the general engine as before (A/B runs)
        const char* s = std::getenv("TGP_REVERSE_FLIP");
        return !(s && s[0] == '0');
    }();
    return on && h->ordering == 1 && h->opt_modal && h->opt_steady2 && !h->is_dense && !h->sde && h->lti && h->p == 1 && h->mv.sR == 0 && missing == nullptr &&
           y != nullptr && !(flags & TGP_REUSE_REDUCE) && !chunk_engine_requested(h) && h->opt_chunk == 0 && !h->hostm.empty() && h->mv.T == h->T &&
           x0_is_stationary(h);
}
// the flipped series where the input lives: *yf, *ff (flags for the forward call)
int flip_series(tgp_handle* h, const double* y, uint32_t flags, const double** yf, uint32_t* ff) {
    *ff = flags;
    if (flags & TGP_IN_DEVICE) {
        HIPCHK(h->bflip_y.ensure((size_t)h->T * sizeof(double)));
        launch_flip(h, y, h->bflip_y.d(), h->T, 1);
        *yf = h->bflip_y.d();
    } else {
        h->flip_host.resize((size_t)h->T);
        std::reverse_copy(y, y + h->T, h->flip_host.begin());
        *yf = h->flip_host.data();
    }
    return TGP_OK;
}
}  // namespace

// ---- wide LTI models (8 < d <= 63; tgp_wide.hip) ----------------------------------------------------------------------------------------
// TGP_WIDE=0: such models on the engines they had before (A/B runs)
bool wide_env_on() {
    static const bool on = [] {
        const char* s = std::getenv("TGP_WIDE");
        return !(s && s[0] == '0');
    }();
    return on;
}
// What every call site of the wide-state engine asks (each adds its own conditions): a wide LTI model bound (`widem`: every block shared, scalar
// observations, Forward), the engine not switched off, no chunked-scan kernels requested, observations given and none missing.
bool wide_eligible(const tgp_handle* h, const double* y, const uint8_t* missing) {
    return wide_env_on() && h->opt_wide && !h->widem.empty() && !chunk_engine_requested(h) && y != nullptr && missing == nullptr;
}
// the bound model as the engine's host plan reads it (the twin of modal_host_model)
void wide_host_model(const tgp_handle* h, tgp_wide::ModelHost& mh) {
    const int d = h->d;
    const size_t dd = (size_t)d * d;
    const double* q = h->widem.data();
    mh.d = d;
    mh.A = q; mh.a = q + dd; mh.Q = q + dd + d; mh.H = q + 2 * dd + d; mh.hh = q[2 * dd + 2 * d]; mh.R = q[2 * dd + 2 * d + 1];
    mh.x0m = h->x0m.data();
    mh.x0P = h->x0P.data();
}

// logpdf and posterior marginals across the chip on the stationary closed loop.  *served = false: the engine declined (nothing the caller must
// undo) -- the dense engine's passes (d > 16) or the general engine serve the call.
static int wide_call(tgp_handle* h, const double* y, uint32_t flags, const double* Rnew, double* mean_out, double* var_out, double* out, bool* served) {
    *served = false;
    if (h->opt_group == 2 || (flags & TGP_REUSE_REDUCE) || h->wide_state < 0) return TGP_OK;
    const bool post = mean_out != nullptr;
    if (post && h->wide_post_state < 0) return TGP_OK;
    if (!h->wide) h->wide = tgp_wide::create();
    tgp_wide::ModelHost mh;
    wide_host_model(h, mh);
    const bool dbg = getenv("TGP_STEADY_DEBUG") != nullptr;
    if (!tgp_wide::plan(h->wide, mh, h->T)) {
        h->wide_state = -1;
        if (dbg) {
            const tgp_wide::Info& in = tgp_wide::last_plan(h->wide);
            fprintf(stderr, "[tgp wide] does not apply: why %d, n0 %d halo %d\n", in.why, in.n0, in.halo);
        }
        return TGP_OK;
    }
    if (post && !tgp_wide::plan_posterior(h->wide, h->T)) {
        h->wide_post_state = -1;
        if (dbg) {
            const tgp_wide::Info& in = tgp_wide::last_plan(h->wide);
            fprintf(stderr, "[tgp wide] posterior does not apply: why %d, n1 %d halo_back %d\n", in.why_post, in.n1, in.halo_back);
        }
        return TGP_OK;
    }
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0, rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    CallTimer tm(h, /*clear=*/false);
    const void* pR = nullptr;
    if (post) TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    double *dm = nullptr, *dv = nullptr;
    TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
    TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
    tgp_wide::Call c;
    c.T = h->T;
    c.y = h->mv.y;
    c.Rnew = static_cast<const double*>(pR);
    c.rnew_per_step = (post && !rshared) ? 1 : 0;
    c.mean = dm;
    c.var = dv;
    c.h_t = h->wide_ht;
    std::string err;
    double lml = 0.0;
    {
        const std::string both = std::string(tgp_wide::kernel_name(h->wide)) + " + k_wide_bwd";      // (the posterior's two kernels under one bracket: the head's copy sits between)
        LaunchScope ls(h, post ? both.c_str() : tgp_wide::kernel_name(h->wide));
        if (tgp_wide::run(h->wide, h->stream, c, &lml, &err) != 0) return h->fail(TGP_EHIP, err);
    }
    TRY(copy_back(h, mean_out, dm, nT, odev));
    TRY(copy_back(h, var_out, dv, nT, odev));
    if (h->profile || (post && !odev)) HIPCHK(hipStreamSynchronize(h->stream));      // (the bracket's closing event; host outputs)
    resolve_profile(h);
    if (dbg) {
        const tgp_wide::Info& in = tgp_wide::last_plan(h->wide);
        fprintf(stderr, "[tgp wide] n0 %d halo %d / %d n1 %d chunks %lld x %lld steps, plan %.3f + %.3f ms\n", in.n0, in.halo, in.halo_back, in.n1, in.chunks, in.chunk_len, in.plan_ms,
                in.plan_post_ms);
    }
    note_served(h, Served::wide, tgp_wide::last_plan(h->wide).n0, lml, out);
    h->wide_state = 1;
    *served = true;
    return TGP_OK;
}

// _filter of a wide LTI model (lgssm.jl:171-187): the forward kernel writes the filtered means of its own steps, the covariances are the head's (host plan)
// and the settled one behind it (one fill kernel).  *served = false: the engine declined.
static int wide_filter_call(tgp_handle* h, const double* y, uint32_t flags, double* m_out, double* P_out, double* lml_out, bool* served) {
    *served = false;
    if (h->opt_group == 2 || (flags & TGP_REUSE_REDUCE) || h->wide_state < 0 || !m_out || !P_out) return TGP_OK;
    if (!h->wide) h->wide = tgp_wide::create();
    const int d = h->d;
    tgp_wide::ModelHost mh;
    wide_host_model(h, mh);
    if (!tgp_wide::plan(h->wide, mh, h->T)) {
        h->wide_state = -1;
        return TGP_OK;
    }
    if (!tgp_wide::filter_ready(h->wide)) return TGP_OK;
    const bool odev = (flags & TGP_OUT_DEVICE) != 0;
    const size_t nm = (size_t)h->T * d * sizeof(double), nP = nm * d;
    CallTimer tm(h, /*clear=*/false);
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    double *dm = nullptr, *dP = nullptr;
    TRY(stage_out(h, h->bo1, m_out, nm, odev, &dm));
    TRY(stage_out(h, h->bo2, P_out, nP, odev, &dP));
    tgp_wide::Call c;
    c.T = h->T;
    c.y = h->mv.y;
    c.fm = dm;
    c.fP = dP;
    c.h_t = h->wide_ht;
    std::string err;
    double lml = 0.0;
    {
        const std::string nm_k = std::string(tgp_wide::kernel_name(h->wide)) + " + k_wide_fill_cov";
        LaunchScope ls(h, nm_k.c_str());
        if (tgp_wide::run(h->wide, h->stream, c, &lml, &err) != 0) return h->fail(TGP_EHIP, err);
    }
    TRY(copy_back(h, m_out, dm, nm, odev));
    TRY(copy_back(h, P_out, dP, nP, odev));
    if (h->profile || !odev) HIPCHK(hipStreamSynchronize(h->stream));
    resolve_profile(h);
    note_served(h, Served::wide, tgp_wide::last_plan(h->wide).n0, lml, lml_out);
    h->wide_state = 1;
    *served = true;
    return TGP_OK;
}

// rand of posterior(model, y) with replaced observation noise of a wide LTI model WITHOUT evaluating that model (tgp_wide::posterior_rand): the forward
// kernel keeping its innovations, k_wide_post_rand on the settled reverse-time transition, the head on the host.  *served = false: the engine or its
// draw plan declined (nothing the caller must undo) -- the caller takes the evaluated route.
static int wide_post_rand_call(tgp_handle* h, const double* y, uint32_t flags, const double* Rnew, const double* eps_t, const double* eps_e, const double* eps_0,
                               double* y_out, bool* served) {
    *served = false;
    if (h->opt_group == 2 || (flags & TGP_REUSE_REDUCE) || h->wide_state < 0 || h->wide_draw_state < 0) return TGP_OK;
    if (!h->wide) h->wide = tgp_wide::create();
    tgp_wide::ModelHost mh;
    wide_host_model(h, mh);
    const bool dbg = getenv("TGP_STEADY_DEBUG") != nullptr;
    if (!tgp_wide::plan(h->wide, mh, h->T)) {
        h->wide_state = -1;
        return TGP_OK;
    }
    if (!tgp_wide::plan_draw(h->wide, h->T)) {
        h->wide_draw_state = -1;
        if (dbg) {
            const tgp_wide::Info& in = tgp_wide::last_plan(h->wide);
            fprintf(stderr, "[tgp wide] posterior draw does not apply: why %d, halo_draw %d\n", in.why_draw, in.halo_draw);
        }
        return TGP_OK;
    }
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0, rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    CallTimer tm(h, /*clear=*/false);
    const void *pR = nullptr, *pet = nullptr, *pee = nullptr;
    TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
    TRY(stage_in(h, h->beps_t, eps_t, (size_t)h->T * h->d * sizeof(double), idev, &pet));
    TRY(stage_in(h, h->beps_e, eps_e, nT, idev, &pee));
    TRY(set_obs(h, y, nullptr, flags));
    tm.inputs_done();
    double* dy = nullptr;
    TRY(stage_out(h, h->bo1, y_out, nT, odev, &dy));
    tgp_wide::Call c;
    c.T = h->T;
    c.y = h->mv.y;
    c.Rnew = static_cast<const double*>(pR);
    c.rnew_per_step = rshared ? 0 : 1;
    c.h_t = h->wide_ht;
    std::string err;
    double lml = 0.0;
    {
        const std::string nm_k = std::string("k_wide_post_rand: ") + tgp_wide::kernel_name(h->wide) + " + k_wide_post_rand";
        LaunchScope ls(h, nm_k.c_str());
        if (tgp_wide::posterior_rand(h->wide, h->stream, c, static_cast<const double*>(pet), static_cast<const double*>(pee), eps_0, dy, &lml, &err) != 0)
            return h->fail(TGP_EHIP, err);
    }
    tm.kernels_done();
    TRY(copy_back(h, y_out, dy, nT, odev));
    if (h->profile || !odev) HIPCHK(hipStreamSynchronize(h->stream));      // (the bracket's closing event; host outputs)
    resolve_profile(h);
    if (dbg) {
        const tgp_wide::Info& in = tgp_wide::last_plan(h->wide);
        fprintf(stderr, "[tgp wide] posterior draw: n0 %d halo %d halo_draw %d chunks %lld x %lld steps, plan %.3f + %.3f ms\n", in.n0, in.halo, in.halo_draw, in.draw_chunks,
                in.draw_chunk_len, in.plan_ms, in.plan_draw_ms);
    }
    if (!(lml == lml)) return TGP_OK;      // (a NaN in the series -- NaN == missing in the mirrors' convention --: the evaluated route serves the draw)
    note_served(h, Served::wide, tgp_wide::last_plan(h->wide).n0, lml, nullptr);
    h->wide_state = 1;
    *served = true;
    return TGP_OK;
}

// logpdf of a Forward LTI model on the one-launch kernels
static int logpdf_lti_one_launch(tgp_handle* h, const double* y, uint32_t flags, double* out, bool* served) {
    *served = false;
    if (!steady2_eligible(h, nullptr, flags)) return TGP_OK;
    TRY(modal_call(h, y, flags, nullptr, nullptr, nullptr, out, served));
    if (*served) return TGP_OK;
    // no well-conditioned modal form (two summands with one length scale, ...): logpdf is the by-product of the filter's forward
    // recursion, which needs none -- ONE kernel on the dense powers of the closed loop (d <= 6; k_filter_one without its outputs)
    if (h->opt_modal && y != nullptr) {
        TRY(smooth_lti_call(h, y, flags, nullptr, nullptr, nullptr, out, served));      // (k_smooth_one's forward half: one sweep, no outputs)
        if (*served) return TGP_OK;
        TRY(filter_lti_call(h, y, flags, nullptr, nullptr, out, served));
    }
    return TGP_OK;
}

