"""GPU tier: the dense engine's passes across the chip (csrc/tgp_dense_chunked.hpp) where tests/test_gpu_dense_chunked.py does not go: the
edges of the three kernel instantiations, the backward repair and decline, the default option set, error reports across chunks, blocks that are per step one
at a time, the edges of the chunk geometry and a handle that is bound again.  Every case asserts tgp_dense_chunk_info, so that a silent fallback cannot
pass a parity assert.  Bars (tests/test_gpu_dense_chunked.py): logpdf 1e-10 relative against oracle/lgssm_ref.py, filtering states 1e-9 of
their scale, marginals 1e-8 against ref.bryson_frazier_marginals (the same recursion, sequential) and 1e-6 against the jittered RTS reference where that
one is used, and _util.against_sequential against option 20 = 0 on the same handle.

Models: _util.random_model with |A| = 0.6 x orthogonal (nothing drawn for the contraction): 96 warm-up steps leave 0.6^96 ~ 5e-22 of a start state with
no observation at all, so the forced geometry (200, 96, 96) passes its checks whatever the series is.  The hand-over distances below are those of the
NumPy restatement (_util.dense_chunk_distances: scripts/dense_chunk_proto.py's forward / backward with p scalar updates per step), computed on the host
from the inputs of each case by `python -m tests.test_gpu_dense_chunked_edges` -- the inputs decide the outcome of a check, not the kernel.

    A  d in {17 ... 64} x p in {1, 16}, T = 1650, (200, 96, 96): dist_f <= 8.1e-16, dist_b <= 7.7e-16 over the 18 cases;
       the product kernel at d = 64 (ApproxPeriodic with 16 harmonics * Matern32, spacing 0.2, noise 0.1), (200, 128, 128): 1.9e-16, 1.2e-15
    B  _strongly_observed (T = 5000, d = 20, p = 16; first guess W0 = 144, 8 chunks of 625), the boundary at s = 2500:
       [s, s + 216) missing ("behind"):        (625, 144, 144): dist_f 5.3e-16 passes, dist_b 1.0 FAILS;  (625, 144, 288): dist_b 8.0e-15 passes
       [s - 158, s + 273) missing ("across"):  (625, 144, 144): dist_f 1.0 FAILS
    D  per-step a / h / Q / A alone, (200, 96, 96): dist_f <= 6.5e-16, dist_b <= 3.7e-16
    E  last chunk of one step, two chunks, chunks of one step, scalar and vector: dist_f <= 6.2e-16, dist_b <= 7.3e-16;
       W = Wb = T: exactly 0 and 0 (every chunk repeats its neighbour's arithmetic from step 0 / from T)

Routing facts these tests turned up (DESIGN 4.6 has them too):
  * tgp_last_error does not carry the step of a non-positive innovation variance ("innovation variance / predicted covariance not positive definite"):
    the two-step case asserts the exception and that the message is the sequential pass's, not the step.
  * A non-positive innovation variance never reaches the caller through a SERVED chunked pass: the chunk's log-determinant runs as a product, the product
    turns negative, its logarithm is NaN, and dk_chunk_close sets bit 8 (non-finite) beside bit 4.  The pass is declined (state -1) and the error is the
    one the sequential pass reports on the same inputs.
  * oracle/components.py builds a product kernel at d = 64 (2 n harmonics-states x Matern32's 2 at n = 16); it has none for the odd edge dimensions.
  * fused_posterior_marginals' sequential Bryson-Frazier tail runs after a backward decline under the DEFAULT option 10 as well (the forward pass across
    the chip has already written the stores it reads): values at the Bryson-Frazier bar, served = 0.

Defects these tests found, fixed with them (csrc/tgp_dense.hip):
  * model_set kept the occupancy looked up for the kernels of the FIRST model's DP (F): a handle bound again across DP = 32 | 48, 64 planned twice or
    half the chunks of a fresh one.  Values were right, the plan was not.
  * posterior_marginals left the record of the declining call in tgp_dense_chunk_info when a declined model went to the per-step chain under the default
    option 10 (attempts = 2 on a call that made none).

Mutations (one scratch build each, run on the device against the group named; every other test of the group passed):
  A  FusedSmoothCfg<48>::NG = 256 / 48 - 1: EQUIVALENT, all of group A passes -- matvec strides its K loop by NG and sums NG partial sums, so four
     slices cover every k as five do (the red / H / aux offsets in LDS follow NG); only the summation order moves.  Instead:
     FusedCfg::HPT - 1 (the last 256 elements of a per-step emission block never reach LDS): test_template_edges[d-16] fails at all nine d.
  B  the backward loop takes a pass whose check failed (ok = no bit 8): both ..._is_repaired_by_a_longer_warm_up and both ..._hands_over_to_the_
     sequential_backward_pass fail.
  B, default options  dk_chunk_close adds the slots in spite of bit 1: test_a_forward_decline_inside_a_posterior_call_with_default_options_counts_
     the_log_likelihood_once fails (the log-likelihood is counted twice).
  D  a_n = g.a[tid]: test_one_block_per_step_and_every_other_shared[a] fails (h, Q, A pass).
  E  `step > g.step0` -> `step >= g.step0` in the forward crossing store: EQUIVALENT, groups A and E pass -- the only chunk it adds a store for is chunk 0,
     whose warm slot dk_chunk_close never reads (it compares from warm + nst).  Instead: n = T / C rounded down: test_geometry_edges fails at
     "last chunk of one step" (one step lost), "two chunks" (n = 1: not tried) and "warm-up of the whole series" (the short last chunk lost), scalar
     and vector.
  F  none needed: both orders failed before model_set forgot the occupancy of another DP (511 chunks of 274 against a fresh handle's 256 of 547 at
     d = 20 -> 40, the reverse at 40 -> 20).

Not covered, and why:
  * the step number of a not-PD report (the ABI does not expose it, above);
  * a backward pass that meets a non-finite value while the forward pass was finite (the records it reads are the forward pass's: no input reaches it
    that the forward check has not seen)."""
import numpy as np
import pytest

from oracle import lgssm_ref as ref

from tests._util import DENSE_TOL_B as TOL_B
from tests._util import DENSE_TOL_F as TOL_F
from tests._util import (against_sequential, dense_chunk_distances, forced, random_model, scalar_dev, sequential, served_once, vector_dev,
                         with_missing)

pytestmark = pytest.mark.gpu
T0, BASE = 1650, (200, 96, 96)          # 9 chunks of 200, the last one of 50
RHO = 0.6


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


# ------------------------------------------------------------------------------------------------ inputs (host only: the proto table reads them too)
def as_scalar(model, Rd):
    """random_model's p = 1 model in ScalarOutputLGC's shapes"""
    return dict(model, kind="scalar", H=model["H"][:, 0, :], h=model["h"][:, 0], R=np.ascontiguousarray(Rd[:, 0]))


def series(rng, T, p, frac=0.15):
    """observations, 15 % of the entries missing, a new noise variance per entry"""
    shape = (T,) if p == 0 else (T, p)
    return rng.standard_normal(shape), rng.random(shape) < frac, rng.uniform(0.01, 0.2, size=shape)


def edge_inputs(d, p):
    rng = np.random.default_rng(7000 + 100 * p + d)
    if p == 1:           # shared blocks, scalar observations
        model, Rd = random_model(rng, T0, d, 1, rho=RHO)
        return (as_scalar(model, Rd), None) + series(rng, T0, 0)
    model, Rd = random_model(rng, T0, d, p, per_step=True, rho=RHO)
    return (model, Rd) + series(rng, T0, p)


def product_inputs():
    from oracle import components as oc
    kernel = ("product", ("approx_periodic", 16, 1.0), ("matern32",))          # 2 x 16 x 2 = 64 states
    model = oc.build_lgssm(kernel, ("regular", 0.0, 0.2, T0), 0.1)
    rng = np.random.default_rng(64)
    y = np.asarray(ref.rand(model, rng.standard_normal((T0, 64)), rng.standard_normal(T0), rng.standard_normal(64))).reshape(T0)
    model = dict(model, R=float(np.ravel(model["R"])[0]) * (0.5 + rng.random(T0)))
    return model, y, rng.random(T0) < 0.15, rng.uniform(0.01, 0.2, size=T0)


STRIDES = ("a", "h", "Q", "A")


def stride_inputs(which):
    """d = 20, p = 2, every block shared but one"""
    d, p = 20, 2
    rng = np.random.default_rng(8000 + STRIDES.index(which))
    model, Rd = random_model(rng, T0, d, p, rho=RHO)
    per_step, _ = random_model(rng, T0, d, p, per_step=True, rho=RHO)
    model[which] = 5.0 * per_step[which] if which in ("a", "h") else per_step[which]      # (offsets of the state's own size)
    return (model, Rd) + series(rng, T0, p)


# name: (T, (C, W, Wb), chunks; 0: the chunks decline the geometry)
GEOMETRIES = {
    "last chunk of one step": (8 * 200 + 1, BASE, 9),
    "two chunks": (T0, (1000, 96, 96), 2),
    "chunks of one step": (T0, (1, 96, 96), T0),
    "warm-up of the whole series": (T0, (200, T0, T0), 9),
    "one chunk": (T0, (T0, 96, 96), 0),
}


def geometry_inputs(kind, T):
    rng = np.random.default_rng(9000 + T + (kind == "vector"))
    if kind == "scalar":
        model, Rd = random_model(rng, T, 18, 1, rho=RHO)
        return (as_scalar(model, Rd), None) + series(rng, T, 0)
    model, Rd = random_model(rng, T, 20, 2, rho=RHO)
    return (model, Rd) + series(rng, T, 2)


# ------------------------------------------------------------------------------------------------ the checks of one case
def not_tried(dm, backward):
    info = dm.handle().dense_chunk_info()
    assert info["served"] == 0 and info["attempts"] == 0 and info["status"] == 0 and info["state"] == 0, info
    return info


def _scale(x):
    return max(1.0, np.abs(x).max())


def check_case(tgp, model, Rd, y, mk, Rn, geometry, served=served_once, rts=False, filt=True, fused=2):
    """logpdf, _filter and logpdf_and_posterior_marginals of one model at one forced geometry: against the reference, against option 20 = 0, with
    `served` asserting the diagnostic after every call.  Scalar models (Rd is None): whole-step mask; vector models: element-wise mask."""
    scalar = Rd is None
    yin = np.where(mk, np.nan, y)
    if scalar:
        dm = scalar_dev(tgp, model, geometry, fused)
        lp_ref = ref.logpdf_missing(model, y, mk)
        m2 = y2 = None
    else:
        dm = vector_dev(tgp, model, Rd, forced(tgp, *geometry, fused=fused))
        m2, y2, comp = with_missing(model, y, mk)
        lp_ref = ref.logpdf(m2, y2) + comp
    lp = tgp.logpdf(dm, yin)
    info = served(dm, False)
    print("logpdf", abs(lp - lp_ref) / abs(lp_ref), info)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)
    if filt:
        fm_ref, fP_ref = ref.filter_missing(model, y, mk) if scalar else ref.filter_(m2, y2)
        fm, fP = tgp._filter(dm, yin)
        served(dm, False)
        np.testing.assert_allclose(fm, fm_ref, rtol=0, atol=1e-9 * _scale(fm_ref))
        np.testing.assert_allclose(fP, fP_ref, rtol=0, atol=1e-9 * _scale(fP_ref))
        fm0, fP0 = sequential(tgp, dm, lambda: tgp._filter(dm, yin))
        np.testing.assert_allclose(fm, fm0, rtol=0, atol=1e-9 * _scale(fm0))
        np.testing.assert_allclose(fP, fP0, rtol=0, atol=1e-9 * _scale(fP0))
    out = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = served(dm, True)
    assert abs(out[0] - lp_ref) <= 1e-10 * abs(lp_ref), (out[0], lp_ref)
    if rts:          # the jittered RTS form of the reference: 1e-6
        pm, pC = ref.marginals(ref.replace_observation_noise_cov(ref.posterior(m2, y2), np.stack([np.diag(r) for r in Rn])))
        pv, tol = np.diagonal(pC, axis1=-2, axis2=-1), 1e-6
    else:            # the same recursion, sequential: 1e-8
        pm, pv = ref.bryson_frazier_marginals(model, y, Rn, missing=mk)
        tol = 1e-8
    print("posterior", np.abs(out[1] - pm).max() / _scale(pm), np.abs(out[2] - pv).max() / _scale(pv), info)
    np.testing.assert_allclose(out[1], pm, rtol=0, atol=tol * _scale(pm))
    np.testing.assert_allclose(out[2], pv, rtol=0, atol=tol * _scale(pv))
    against_sequential(out, sequential(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, yin, Rn)))
    return dm, yin, out, info


# ------------------------------------------------------------------------------------------------ A. template edges
@pytest.mark.parametrize("p", (1, 16))
@pytest.mark.parametrize("d", (17, 31, 32, 33, 47, 48, 49, 63, 64))
def test_template_edges(tgp, d, p):
    """d on both sides of DP = 32, 48, 64 and at the ends of the range; p = 1 (shared blocks, scalar observations, marginals against the sequential
    Bryson-Frazier form) and p = 16 (every block per step, marginals against the jittered RTS form); a new noise variance per step"""
    model, Rd, y, mk, Rn = edge_inputs(d, p)
    *_, info = check_case(tgp, model, Rd, y, mk, Rn, BASE, rts=p > 1)
    assert info["chunks"] == 9 and info["C"] == 200 and info["W"] == 96 and info["Wb"] == 96, info


def test_product_kernel_at_the_last_template_edge(tgp):
    """ApproxPeriodicKernel (16 harmonics) * Matern32Kernel: d = 64 = DP, the one product kernel oracle/components.py has at a template edge"""
    model, y, mk, Rn = product_inputs()
    assert len(model["x0m"]) == 64
    *_, info = check_case(tgp, model, None, y, mk, Rn, (200, 128, 128))
    assert info["chunks"] == 9, info


# ------------------------------------------------------------------------------------------------ B. backward repair, backward decline, default options
W0 = 144          # the first guess of _strongly_observed (chunk_estimate: the closed loop squared 7 times, plus an eighth); asserted on the device below


def repair_inputs():
    from tests.test_gpu_dense_chunked import _strongly_observed
    rng = np.random.default_rng(11)
    T, p = 5000, 16
    model, Rd = _strongly_observed(rng, T)
    y = ref.rand(model, rng.standard_normal((T, 20)), rng.standard_normal((T, p)), rng.standard_normal(20))
    C = 625                                  # 8 chunks of >= 4 W0
    s = 4 * C
    behind = np.zeros((T, p), dtype=bool)    # 3 W0 / 2 steps BEHIND a boundary: the forward warm-up in front of it sees every observation; the backward
    behind[s:s + (3 * W0) // 2] = True       # warm-up of W0 steps sees none (its pair stays 0), the one of 2 W0 steps has W0 / 2 observed steps
    across = np.zeros((T, p), dtype=bool)    # (tests/test_gpu_dense_chunked.py) 1.1 W0 in front of the boundary, 1.9 W0 behind: defeats W0 forwards
    across[s - (11 * W0) // 10:s + (19 * W0) // 10] = True
    Rn = rng.uniform(0.01, 0.2, size=(T, p))
    return model, Rd, y, dict(behind=behind, across=across), Rn, C


@pytest.fixture(scope="module")
def repair(tgp):
    model, Rd, y, masks, Rn, C = repair_inputs()
    pilot = vector_dev(tgp, model, Rd, {})
    tgp.logpdf(pilot, y)
    first = pilot.handle().dense_chunk_info()
    assert first["served"] == 1 and first["attempts"] == 1 and first["W"] == W0 and first["C"] == C and first["chunks"] == 8, first
    cache = {}

    def refs(name, rts=False):
        if name not in cache:
            m2, y2, comp = with_missing(model, y, masks[name])
            cache[name] = dict(m2=m2, y2=y2, lp=ref.logpdf(m2, y2) + comp, bf=ref.bryson_frazier_marginals(model, y, Rn, missing=masks[name]))
        c = cache[name]
        if rts and "rts" not in c:
            pm, pC = ref.marginals(ref.replace_observation_noise_cov(ref.posterior(c["m2"], c["y2"]), np.stack([np.diag(r) for r in Rn])))
            c["rts"] = (pm, np.diagonal(pC, axis1=-2, axis2=-1))
        return c
    return model, Rd, y, masks, Rn, refs


def _values(out, r, key, tol):
    assert abs(out[0] - r["lp"]) <= 1e-10 * abs(r["lp"]), (out[0], r["lp"])
    pm, pv = r[key]
    print(key, np.abs(out[1] - pm).max() / _scale(pm), np.abs(out[2] - pv).max() / _scale(pv))
    np.testing.assert_allclose(out[1], pm, rtol=0, atol=tol * _scale(pm))
    np.testing.assert_allclose(out[2], pv, rtol=0, atol=tol * _scale(pv))


@pytest.mark.parametrize("fused", (2, None), ids=("option 10 = 2", "default options"))
def test_a_backward_check_that_fails_is_repaired_by_a_longer_warm_up(tgp, repair, fused):
    """host restatement: forwards W0 passes, backwards W0 fails and 2 W0 passes (B in the table above)"""
    model, Rd, y, masks, Rn, refs = repair
    yin = np.where(masks["behind"], np.nan, y)
    dm = vector_dev(tgp, model, Rd, {} if fused is None else {tgp._lib.OPT_DENSE_FUSED: fused})
    out = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = dm.handle().dense_chunk_info()
    print(info)
    assert info["served"] == 1 and info["status"] == 0 and info["state"] == 1 and info["chunks"] == 8, info
    assert info["attempts"] >= 3 and info["W"] == W0 and info["Wb"] > W0, info          # 1 forwards + >= 2 backwards
    assert info["dist_f"] <= TOL_F and info["dist_b"] <= TOL_B, info
    _values(out, refs("behind"), "bf", 1e-8)
    again = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    later = dm.handle().dense_chunk_info()
    assert later["served"] == 1 and later["attempts"] == 2 and later["W"] == W0 and later["Wb"] == info["Wb"], later      # (the bound model remembers Wb)
    assert later["dist_b"] <= TOL_B, later
    _values(again, refs("behind"), "bf", 1e-8)


@pytest.mark.parametrize("fused", (2, None), ids=("option 10 = 2", "default options"))
def test_a_backward_check_that_fails_under_a_forced_warm_up_hands_over_to_the_sequential_backward_pass(tgp, repair, fused):
    """the sequential Bryson-Frazier pass runs on the stores the forward pass across the chip wrote: same bars; no attempt afterwards"""
    model, Rd, y, masks, Rn, refs = repair
    L = tgp._lib
    yin = np.where(masks["behind"], np.nan, y)
    dm = vector_dev(tgp, model, Rd, {L.OPT_DENSE_WARMUP_BACK: W0, **({} if fused is None else {L.OPT_DENSE_FUSED: fused})})
    out = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = dm.handle().dense_chunk_info()
    print(info)
    assert info["served"] == 0 and info["status"] & 2 and not info["status"] & 1 and info["state"] == -1 and info["attempts"] == 2, info
    assert info["dist_f"] <= TOL_F and info["dist_b"] > TOL_B and info["Wb"] == W0, info
    _values(out, refs("behind"), "bf", 1e-8)
    again = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    later = dm.handle().dense_chunk_info()
    assert later["served"] == 0 and later["attempts"] == 0 and later["state"] == -1, later
    if fused == 2:       # the sequential Bryson-Frazier passes
        _values(again, refs("behind"), "bf", 1e-8)
    else:                # the per-step chain (the reference's jittered RTS form)
        _values(again, refs("behind", rts=True), "rts", 1e-6)


def test_a_forward_decline_inside_a_posterior_call_with_default_options_counts_the_log_likelihood_once(tgp, repair):
    """forced W0 against the stretch that defeats it (B in the table above): fused_filter returns TGP_EUNSUPPORTED, the per-step chain serves the call"""
    model, Rd, y, masks, Rn, refs = repair
    yin = np.where(masks["across"], np.nan, y)
    dm = vector_dev(tgp, model, Rd, {tgp._lib.OPT_DENSE_WARMUP: W0})
    out = tgp.logpdf_and_posterior_marginals(dm, yin, Rn)
    info = dm.handle().dense_chunk_info()
    print(info)
    assert info["served"] == 0 and info["status"] & 1 and info["attempts"] == 1 and info["state"] == -1 and info["dist_f"] > TOL_F, info
    _values(out, refs("across", rts=True), "rts", 1e-6)


# ------------------------------------------------------------------------------------------------ C. errors
def _error_model():
    rng = np.random.default_rng(10_000)
    model, Rd = random_model(rng, T0, 20, 2, rho=RHO)
    y, _, Rn = series(rng, T0, 2)
    return model, Rd.copy(), y, Rn


def _outcome(fn):
    try:
        return "value", fn()
    except Exception as e:      # noqa: BLE001  (compared with the sequential pass's below)
        return type(e), str(e)


def _calls(tgp, y, Rn):
    return (("logpdf", lambda dm: tgp.logpdf(dm, y)), ("_filter", lambda dm: tgp._filter(dm, y)),
            ("posterior", lambda dm: tgp.logpdf_and_posterior_marginals(dm, y, Rn)))


@pytest.mark.parametrize("steps", ((590,), (590, 1190)), ids=("one step", "two steps in different chunks"))
def test_a_non_positive_innovation_variance_is_reported_as_the_sequential_pass_reports_it(tgp, steps):
    """R[590, 1] = -50: ten steps in front of the boundary at 600 -- an own step of chunk 2 and a warm-up step of chunk 3.  The message does not carry
    the step (tgp_last_error): with two bad steps the exception and its text are compared with the sequential pass's."""
    from temporalgps_jl_amd import _lib
    model, Rd, y, Rn = _error_model()
    for t in steps:
        Rd[t, 1] = -50.0
    for name, call in _calls(tgp, y, Rn):
        dm = vector_dev(tgp, model, Rd, forced(tgp, *BASE))          # (a fresh handle per call: a declined model is not tried again)
        with pytest.raises(_lib.NotPositiveDefinite) as chunked:
            call(dm)
        info = dm.handle().dense_chunk_info()
        print(name, info)
        assert info["attempts"] == 1 and info["status"] & 4, info          # the chunks ran and saw it
        assert info["served"] == 0 and info["status"] & 8 and info["state"] == -1, info      # (log of a negative product: see the file's docstring)
        with pytest.raises(_lib.NotPositiveDefinite) as seq:
            sequential(tgp, dm, lambda: call(dm))
        assert str(chunked.value) == str(seq.value)


def test_a_non_finite_observation_declines_the_pass(tgp):
    model, Rd, y, Rn = _error_model()
    y[700, 0] = np.inf
    for name, call in _calls(tgp, y, Rn):
        dm = vector_dev(tgp, model, Rd, forced(tgp, *BASE))
        kind, got = _outcome(lambda: call(dm))
        info = dm.handle().dense_chunk_info()
        print(name, kind, info)
        assert info["served"] == 0 and info["status"] & 8 and info["state"] == -1 and info["attempts"] == 1, info
        hd = dm.handle()
        hd.set_option(tgp._lib.OPT_DENSE_CHUNKED, 0)
        kind0, want = _outcome(lambda: call(dm))
        assert hd.dense_chunk_info()["served"] == 0 and hd.dense_chunk_info()["attempts"] == 0
        assert kind == kind0
        if kind == "value":
            got, want = (tuple(np.asarray(v) for v in (x if isinstance(x, tuple) else (x,))) for x in (got, want))
            assert len(got) == len(want) and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(got, want)), name
            assert not np.isfinite(got[0]).all(), name          # (the call does not hide it)
        else:
            assert got == want


# ------------------------------------------------------------------------------------------------ D. mixed strides
@pytest.mark.parametrize("which", STRIDES)
def test_one_block_per_step_and_every_other_shared(tgp, which):
    """a per-step offset a alone (a mean function), h alone (H shared: the per-step prefetch at sH = 0), Q alone, A alone -- on chunks that start mid-series"""
    model, Rd, y, mk, Rn = stride_inputs(which)
    assert all((model[k].shape[0] == T0) == (k == which) for k in ("A", "a", "Q", "H", "h"))
    *_, info = check_case(tgp, model, Rd, y, mk, Rn, BASE, filt=False)
    assert info["chunks"] == 9 and info["C"] == 200, info


# ------------------------------------------------------------------------------------------------ E. geometry
@pytest.mark.parametrize("kind", ("scalar", "vector"))
@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_geometry_edges(tgp, name, kind):
    T, geometry, chunks = GEOMETRIES[name]
    model, Rd, y, mk, Rn = geometry_inputs(kind, T)
    *_, info = check_case(tgp, model, Rd, y, mk, Rn, geometry, served=served_once if chunks else not_tried)
    if chunks:
        assert info["chunks"] == chunks and (info["C"], info["W"], info["Wb"]) == geometry, info
    if name == "warm-up of the whole series":          # every chunk starts at step 0 and every backward chunk at T: the same arithmetic as its neighbour
        assert info["dist_f"] == 0.0 and info["dist_b"] == 0.0, info


def test_more_chunks_than_the_close_kernel_takes_are_declined(tgp):
    """C = 1 at T = 66 000: n > 65 536"""
    T = 66_000
    rng = np.random.default_rng(9999)
    model, Rd = random_model(rng, T, 18, 1, rho=RHO)
    model = as_scalar(model, Rd)
    y, mk, _ = series(rng, T, 0)
    dm = scalar_dev(tgp, model, (1, 96, 96))
    lp = tgp.logpdf(dm, np.where(mk, np.nan, y))
    not_tried(dm, False)
    lp_ref = ref.logpdf_missing(model, y, mk)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)


# ------------------------------------------------------------------------------------------------ F. handle reuse
def _long_model(seed, T, d):
    """shared A, a, Q, h; H and R per step: the first guess of a model with a per-step block is 64 steps, nothing is estimated"""
    rng = np.random.default_rng(seed)
    model, _ = random_model(rng, 1, d, 1, rho=RHO)
    H, R = rng.standard_normal((T, d)) / np.sqrt(d), rng.uniform(0.05, 0.3, size=T)
    return dict(model, kind="scalar", T=T, H=H, h=model["h"][:, 0], R=R), rng.standard_normal(T)


def _rebind(monkeypatch, tgp, hd, dm):
    """tgp_model_set on a handle that already holds a model, as LGSSM.handle() calls it"""
    with monkeypatch.context() as mp:
        mp.setattr(tgp._lib, "Handle", lambda device=0: hd)
        assert dm.handle() is hd
    return dm


@pytest.mark.parametrize("order", ((20, 40), (40, 20)))
def test_a_handle_bound_again_plans_its_chunks_as_a_fresh_one(tgp, monkeypatch, order):
    """DP = 32 has two resident workgroups per CU, DP = 48 one: T / (4 x 64) = 546 exceeds both 256 and 512 chunks, so the plan shows which occupancy
    it was made with.  The occupancy is looked up once per DP (model_set forgets it when DP changes)."""
    T = 140_000
    (ma, ya), (mb, yb) = _long_model(order[0], T, order[0]), _long_model(order[1], T, order[1])
    first = scalar_dev(tgp, ma)
    tgp.logpdf(first, ya)
    assert first.handle().dense_chunk_info()["served"] == 1
    again = _rebind(monkeypatch, tgp, first.handle(), scalar_dev(tgp, mb))
    lp = tgp.logpdf(again, yb)
    info = again.handle().dense_chunk_info()
    fresh = scalar_dev(tgp, mb)
    lp_fresh = tgp.logpdf(fresh, yb)
    want = fresh.handle().dense_chunk_info()
    print(info, want)
    assert want["served"] == 1 and want["status"] == 0 and want["dist_f"] <= TOL_F, want
    assert info["served"] == 1 and (info["chunks"], info["C"], info["W"]) == (want["chunks"], want["C"], want["W"]), (info, want)
    assert lp == lp_fresh


def test_a_declined_verdict_does_not_survive_a_rebind(tgp, monkeypatch):
    model, Rd, y, _ = _error_model()
    bad = y.copy()
    bad[700, 0] = np.inf
    first = vector_dev(tgp, model, Rd, forced(tgp, *BASE))
    _outcome(lambda: tgp.logpdf(first, bad))
    assert first.handle().dense_chunk_info()["state"] == -1
    rng = np.random.default_rng(10_001)
    other, Rd2 = random_model(rng, T0, 40, 2, rho=RHO)
    again = _rebind(monkeypatch, tgp, first.handle(), vector_dev(tgp, other, Rd2, forced(tgp, *BASE)))
    assert again.handle().dense_chunk_info()["state"] == 0
    y2 = rng.standard_normal((T0, 2))
    lp = tgp.logpdf(again, y2)
    served_once(again, False)
    lp_ref = ref.logpdf(other, y2)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)


# ------------------------------------------------------------------------------------------------ the host restatement's verdicts (the docstring's table)
def proto_table():
    def row(label, model, y, mk, geometry):
        df, db = dense_chunk_distances(model, y, mk, *geometry)
        print(f"{label}: {geometry} dist_f {df:.2e} dist_b {db:.2e}", flush=True)
    for d in (17, 31, 32, 33, 47, 48, 49, 63, 64):
        for p in (1, 16):
            model, _, y, mk, _ = edge_inputs(d, p)
            row(f"A d = {d} p = {p}", model, y, mk, BASE)
    model, y, mk, _ = product_inputs()
    row("A product kernel d = 64", model, y, mk, (200, 128, 128))
    model, _, y, masks, _, C = repair_inputs()
    row("B behind", model, y, masks["behind"], (C, W0, W0))
    row("B behind", model, y, masks["behind"], (C, W0, 2 * W0))
    row("B across", model, y, masks["across"], (C, W0, W0))
    for which in STRIDES:
        model, _, y, mk, _ = stride_inputs(which)
        row(f"D per-step {which}", model, y, mk, BASE)
    for name, (T, geometry, chunks) in GEOMETRIES.items():
        for kind in ("scalar", "vector"):
            if chunks:
                model, _, y, mk, _ = geometry_inputs(kind, T)
                row(f"E {name} ({kind})", model, y, mk, geometry)


if __name__ == "__main__":
    proto_table()
