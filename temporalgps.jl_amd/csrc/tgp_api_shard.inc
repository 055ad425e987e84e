// Part of tgp_api.hip (included there, one translation unit): time shards: the scan-element exchange of the general engine and of the stationary-gain engine.
extern "C" {

int tgp_elem_size(int kind, int d) { return kind == 0 ? felem_size(d) : aelem_size(d); }

int tgp_segment_reduce(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, double* elem_out) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h));
    TRY(scan_only(h, "tgp_segment_reduce"));
    if (!elem_out) return h->fail(TGP_EINVAL, "elem_out is NULL");
    CallTimer tm(h);
    TRY(set_obs(h, y, missing, flags));
    tm.inputs_done();
    TRY(forward_reduce(h, flags));
    TRY(scan_total_to_host(h, h->F, elem_out));
    tm.kernels_done();
    return tm.finish();
}

// ---- device-resident exchange (include/tgp_hip.h): every phase only ENQUEUES work on the handle's stream
int tgp_shard_slot_size(int phase, int d) {
    if (d < 1 || d > 16) return 0;
    return phase == 0 ? felem_size(d) : aelem_size(d) + state_size(d);
}

int tgp_shard_reduce(tgp_handle* h, const double* y, const uint8_t* missing, uint32_t flags, double* slot_dev) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h));
    TRY(scan_only(h, "tgp_shard_reduce"));
    if (!slot_dev) return h->fail(TGP_EINVAL, "slot_dev is NULL");
    CallTimer tm(h);                                   // clears the result / flag words for the whole multi-phase call
    h->fold_valid = false;
    TRY(set_obs(h, y, missing, flags));
    TRY(forward_reduce(h, flags));
    const double* e = nullptr;
    TRY(scan_total_dev(h, h->F, &e));
    HIPCHK(hipMemcpyAsync(slot_dev, e, (size_t)h->F.NC * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return TGP_OK;
}

int tgp_shard_fold(tgp_handle* h, const double* gathered_dev, int world, int rank) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h));
    TRY(scan_only(h, "tgp_shard_fold"));
    if (!gathered_dev || world < 1 || rank < 0 || rank >= world) return h->fail(TGP_EINVAL, "bad gathered buffer / world / rank");
    if (!h->reduce_valid) return h->fail(TGP_EINVAL, "tgp_shard_fold needs a preceding tgp_shard_reduce");
    HIPCHK(h->bx0fold.ensure((size_t)state_size(h->d) * sizeof(double)));
    {
        LaunchScope ls(h, "k_fold<filter>");
        h->kt->fold(kFilter, gathered_dev, felem_size(h->d), 0, rank, 1, h->bx0.d(), h->bx0fold.d(), h->stream);
    }
    h->fold_valid = true;
    return TGP_OK;
}

int tgp_shard_logpdf(tgp_handle* h, double* stats_dev) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h));
    TRY(scan_only(h, "tgp_shard_logpdf"));
    if (!stats_dev) return h->fail(TGP_EINVAL, "stats_dev is NULL");
    if (!h->fold_valid || !h->reduce_valid) return h->fail(TGP_EINVAL, "tgp_shard_logpdf needs tgp_shard_reduce + tgp_shard_fold first");
    FilterOut fo{};
    TRY(forward_apply(h, 0, fo, h->bx0fold.d()));
    hipLaunchKernelGGL(k_pack_stats, dim3(1), dim3(64), 0, h->stream, h->result.d(), stats_dev);
    HIPCHK(hipGetLastError());
    return TGP_OK;
}

int tgp_shard_smoother_forward(tgp_handle* h, double* slot_dev) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h));
    TRY(scan_only(h, "tgp_shard_smoother_forward"));
    if (!slot_dev) return h->fail(TGP_EINVAL, "slot_dev is NULL");
    if (h->ordering != 0) return h->fail(TGP_EUNSUPPORTED, "posterior of a Reverse-ordered model is not implemented on the device");
    if (!h->fold_valid || !h->reduce_valid) return h->fail(TGP_EINVAL, "tgp_shard_smoother_forward needs tgp_shard_reduce + tgp_shard_fold first");
    TRY(smoother_forward_impl(h, TGP_REUSE_REDUCE, h->bx0fold.d()));
    const double* e = nullptr;
    TRY(scan_total_dev(h, h->Rv, &e));
    const size_t na = (size_t)aelem_size(h->d), ns = (size_t)state_size(h->d);
    HIPCHK(hipMemcpyAsync(slot_dev, e, na * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(hipMemcpyAsync(slot_dev + na, h->F.fin, ns * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    return TGP_OK;
}

int tgp_shard_smoother_backward(tgp_handle* h, const double* gathered_dev, int world, int rank, const double* Rnew, uint32_t flags,
                                double* mean_out, double* var_out, double* lml_out) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h));
    TRY(scan_only(h, "tgp_shard_smoother_backward"));
    if (!h->smoother_valid) return h->fail(TGP_EINVAL, "tgp_shard_smoother_backward needs a preceding tgp_shard_smoother_forward");
    if (!gathered_dev || world < 1 || rank < 0 || rank >= world) return h->fail(TGP_EINVAL, "bad gathered buffer / world / rank");
    if (!Rnew || !mean_out || !var_out) return h->fail(TGP_EINVAL, "null Rnew / output");
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0;
    const bool rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * h->p * sizeof(double);
    CallTimer tm(h, /*clear=*/false);
    const void* pR = nullptr;
    TRY(stage_in(h, h->bRnew, Rnew, rshared ? (size_t)h->p * sizeof(double) : nT, idev, &pR));
    tm.inputs_done();
    // x_{T_r | T}: the last rank's final filtered state pulled back through the smoother elements of ranks W-1 .. rank+1
    const int64_t slot = aelem_size(h->d) + state_size(h->d);
    HIPCHK(h->bx0r.ensure((size_t)state_size(h->d) * sizeof(double)));
    {
        LaunchScope ls(h, "k_fold<smoother>");
        h->kt->fold(kAffineCov, gathered_dev, slot, world - 1, world - 1 - rank, -1,
                    gathered_dev + (int64_t)(world - 1) * slot + aelem_size(h->d), h->bx0r.d(), h->stream);
    }
    double *dm = nullptr, *dv = nullptr;
    TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
    TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
    TRY(smoother_backward_impl(h, h->bx0r.d(), (const double*)pR, rshared ? 0 : 1, dm, dv));
    tm.kernels_done();
    TRY(copy_back(h, mean_out, dm, nT, odev));
    TRY(copy_back(h, var_out, dv, nT, odev));
    return tm.finish(lml_out);
}

// ---- time shards on the stationary-gain engine (tgp_steady.hpp: ShardDev) ----------------------------------------------------------------
int tgp_shard_steady_slot_size(int d) { return tgp_steady::supports(d) ? (int)tgp_steady::shard_slot_size(d) : 0; }

int tgp_shard_steady_begin(tgp_handle* h, const double* y, uint32_t flags, int first, int last, int posterior, double* slot_dev) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    h->shard2_open = false;
    if (!slot_dev) return h->fail(TGP_EINVAL, "slot_dev is NULL");
    if (!steady2_eligible(h, nullptr, flags) || h->T <= tgp_steady::kTile)
        return h->fail(TGP_EUNSUPPORTED, "tgp_shard_steady_begin: not a model / segment of the stationary-gain engine (use the tgp_shard_* protocol of the general engine)");
    CallTimer tm(h, /*clear=*/false);
    TRY(set_obs(h, y, nullptr, flags));
    tgp_steady::ShardDev sd;
    sd.first = first ? 1 : 0;
    sd.last = last ? 1 : 0;
    sd.post = posterior ? 1 : 0;
    sd.slot = slot_dev;
    TRY(steady2_enqueue(h, nullptr, false, nullptr, nullptr, false, &sd, 0));
    h->shard2_first = sd.first;
    h->shard2_last = sd.last;
    h->shard2_post = sd.post;
    h->shard2_open = true;
    return TGP_OK;
}

int tgp_shard_steady_finish(tgp_handle* h, const double* gathered_dev, int world, int rank, const double* Rnew, uint32_t flags, double* mean_out,
                            double* var_out, double* lml_out, int* served) {
    StreamGuard stream_guard_(h);
    TRY(check_ready(h, /*general=*/false));
    if (!h->shard2_open) return h->fail(TGP_EINVAL, "tgp_shard_steady_finish needs a preceding tgp_shard_steady_begin");
    h->shard2_open = false;
    if (!gathered_dev || world < 1 || world > 64 || rank < 0 || rank >= world || !served) return h->fail(TGP_EINVAL, "bad gathered buffer / world / rank / served");
    const bool post = h->shard2_post != 0;
    if (post && (!Rnew || !mean_out || !var_out)) return h->fail(TGP_EINVAL, "null Rnew / output");
    const bool idev = (flags & TGP_IN_DEVICE) != 0, odev = (flags & TGP_OUT_DEVICE) != 0;
    const bool rshared = (flags & TGP_SHARED_R) != 0;
    const size_t nT = (size_t)h->T * sizeof(double);
    CallTimer tm(h, /*clear=*/false);
    tgp_steady::ShardDev sd;
    sd.first = h->shard2_first;
    sd.last = h->shard2_last;
    sd.post = h->shard2_post;
    sd.gathered = gathered_dev;
    sd.world = world;
    sd.rank = rank;
    const void* pR = nullptr;
    double *dm = nullptr, *dv = nullptr;
    if (post) {
        TRY(stage_in(h, h->bRnew, Rnew, rshared ? sizeof(double) : nT, idev, &pR));
        TRY(stage_out(h, h->bo1, mean_out, nT, odev, &dm));
        TRY(stage_out(h, h->bo2, var_out, nT, odev, &dv));
    }
    tm.inputs_done();
    TRY(steady2_enqueue(h, (const double*)pR, !rshared, dm, dv, false, &sd, 1));
    tm.kernels_done();
    if (post) {
        TRY(copy_back(h, mean_out, dm, nT, odev));
        TRY(copy_back(h, var_out, dv, nT, odev));
    }
    TRY(tm.finish(lml_out));
    *served = h->host_result[6] == tgp_steady::kStatusRan ? 1 : 0;
    drop_reduction(h);
    h->fold_valid = false;
    return TGP_OK;
}

