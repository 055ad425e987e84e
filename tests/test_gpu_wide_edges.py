"""GPU tier: the wide-state engine (8 < d <= 63; csrc/tgp_wide.hip) at every kernel-family edge and over the chunk geometries its plan produces.

State dimensions.  The observer is output d >> 4 of lane d & 15; the components per lane (NB) and the table width change at d = 15/16, 31/32 and 47/48.
tests/_util.py BOUNDARY_KERNELS has a model for d = 17 (one component in the second register), 31, 32, 33, 47, 48, 49 (the two upper form boundaries), 54 (the
LDS form) and 63 (the observer in the wave's last lane).  Every operation of the engine runs at every one of them against the references and bars of
tests/test_gpu_wide.py, test_gpu_wide_draw.py and test_gpu_wide_adjoint.py (the adjoint's cases at d = 31, 32, 47, 48, 63 are in that file's KERNELS).

Kernel names.  A profile label names the FORM the plan chose, and the form fixes every kernel of the call (csrc/tgp_wide.hip forward / backward):
    "k_wide_lml4<16>"  k_wide_lml4<., 1> and k_wide_bwd4<1, .>   (d <= 15)         "k_wide_lml<32>"  k_wide_lml<32>, k_wide_bwd<32, .>  (TGP_WIDE_DPP=0, d <= 31)
    "k_wide_lml4"      k_wide_lml4<., 2> and k_wide_bwd4<2, .>   (d <= 31)         "k_wide_lml<64>"  k_wide_lml<64>, k_wide_bwd<64, .>  (d >= 48; TGP_WIDE_DPP=0, d >= 32)
    "k_wide_lml4<48>"  k_wide_lml4<., 3> and k_wide_bwd4<3, .>   (d <= 47)
logpdf is the label alone (KEEP = false); "+ k_wide_bwd" the posterior (KEEP = true, ADJ = false); "+ k_wide_fill_cov" _filter; "k_wide_adjoint: ... + k_wide_bwd +
k_wide_gram" the adjoint (ADJ = true); "k_wide_post_rand: ... + k_wide_post_rand" the posterior draw; "k_wide_rand" rand.  Every test asserts the whole label.

Chunk geometry.  tgp_wide_plan's info = [why, n0, halo, why_post, n1, halo_back, chunks, chunk_len] chooses the lengths and is asserted for what was hit:
one chunk of exactly 64 steps, the first partial 16-block behind it, a last chunk of 1 ... 15 steps, forced counts of 1, 2, 3, 5, 7 chunks (TGP_WIDE_CHUNKS in a child
process: chunks several halos long, one to three invalid rows in the last DPP wave), exactly 4096 chunks longer than their warm-up, and more than 4096 chunks.
NOTE on the small lengths: the plan makes no chunk shorter than max(64, halo / 2) steps, and these models' halos are 272 ... 336, so n0 + 128, n0 + 129 and
n0 + 3 * 64 + 1 are still ONE chunk (of 128, 129, 193 steps: two, two and three 64-step blocks plus a partial one); the two-chunk case is 2 * max(64, halo / 2) + 1.
The long series are held against the C oracle's run-time path (oracle/seq_kalman.c; tests/test_oracle_c.py pins it to the NumPy restatement), not against
the project's own dense engine.

Bounds that were measured (CPU, on the cases of this file: spacing 0.1, noise 0.1), not inherited:
  * The NumPy prototype of the algorithm (scripts/wide_proto.py, 5 chunks) against the dense GP on the model's own covariance function, T = 2500, per-step Rnew,
    max(mean error / max(1, |mean|), variance error / max(1, var)):
        d = 17: 6.6e-15    d = 31: 8.8e-15    d = 32: 8.5e-15    d = 33: 2.6e-14    d = 47: 8.9e-15
        d = 48: 8.8e-15    d = 49: 1.3e-14    d = 54: 1.2e-14    d = 63: 3.3e-14      (its logpdf: within 5.6e-15 relative of ref.logpdf at every d)
    All within 1e-9, so the dense-GP bar stays 1e-8 at every new d (DENSE_GP_BAR).
  * The posterior draw at d = 17: scripts/wide_draw_proto.py stands 2.4e-15 (relative to the path's largest value) from ref.posterior + ref.rand on draw_case(17)
    (T = 3000, 5 chunks) -- far more than a decade inside 1e-9, the bar of tgp_rand, which
    d = 17 therefore gets as d = 9 and 12 did; d = 33, 48 and 63 get 1e-6, that file's bar for d >= 28.
  * The oracle's zero-draw restatement (ref.posterior + ref.rand with all draws zero) from the dense GP's posterior mean on draw_case(d), absolute:
        d = 17: 7.59e-9    d = 33: 3.10e-8    d = 48: 2.26e-8    d = 63: 5.59e-8
    The kernel's zero draw gets ten times that (ORACLE_ZERO_DRAW_FROM_DENSE_GP).
  * The C oracle's run-time path against the NumPy restatement at d = 63, T = 1500 (tests/test_oracle_c.py): logpdf 0.0 relative, filtered means 9.8e-16, filtered
    covariances 3.0e-16, RTS marginals 1.3e-15 / 2.6e-15 -- the 1e-12 / 1e-10 bounds of that test stand as set.

Mutation checks (one-line breaks of csrc/tgp_wide.hip in a scratch copy; this file on an MI355X against each):
  * `obs_o = (d - 1) >> 4` (both DPP kernels): RUN.  test_logpdf_of_a_second_length_at_the_boundary_dimensions[32] fails, the other eight d pass -- d = 32 is the
    one boundary dimension whose observer output moves (d = 48 runs the LDS form, which has no obs_o).
  * row `16 * o + p + 1` in load_rows: RUN.  test_logpdf_of_a_second_length_at_the_boundary_dimensions[17], [31], [32], [33], [47] fail -- every d of the DPP
    forms --, d = 48, 49, 54, 63 (LDS form) pass.
  * dropping `if (g.s1 > T) g.s1 = T` in row_geom: ARGUED FROM THE CODE, NOT RUN -- the break makes the last chunk read y[t] and write rout[t], mout[t d + .]
    for T <= t < s1, past the end of device buffers, which is not to be provoked on a GPU.  Without the clamp the last valid row has s1 = s0 + chunk_len > T
    whenever T - n0 is no multiple of chunk_len; fwd_step4's `live = t < g.s1` and `own` then hold for s1 - T steps behind the series' end, whose squared
    "innovations" enter ssq and so the logpdf -- a relative change of order (s1 - T) / T, against a bar of 1e-10.  Cases with such a last chunk: every
    T = 2500 / 3000 case of this file (d = 12, T = 3000: 21 chunks of 139 steps for 2908, eleven steps over), the forced 3-, 5- and 7-chunk children,
    test_a_last_chunk_of_a_few_steps_against_the_c_oracle (chunk_len - 15 steps over) and both long-series tests (five steps short by construction)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref
from oracle import seq_kalman as sk
from tests._util import BOUNDARY_KERNELS, ROOT, dense_gp_posterior, device_model, kernels_of, wide_plan
from tests._util import wide_form_label as form_label

pytestmark = pytest.mark.gpu

KERNELS = {
    9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))),
    12: ("product", ("matern32",), ("approx_periodic", 3, 1.0)),
    28: ("product", ("approx_periodic", 7, 1.0), ("matern32",)),
    42: ("product", ("approx_periodic", 7, 1.0), ("matern52",)),
    **BOUNDARY_KERNELS,
}
EDGES = sorted(BOUNDARY_KERNELS)
GEOMETRY_D = (12, 28, 42, 54)      # NB = 1, 2, 3 and the LDS form
# (the prototype stands within 1e-9 of the dense GP at every one of these d -- the table above --, so the bar of tests/test_gpu_wide.py holds)
DENSE_GP_BAR = {d: 1e-8 for d in KERNELS}
REL_DRAW_RESTATEMENT = {17: 1e-9, 33: 1e-6, 48: 1e-6, 63: 1e-6}
ORACLE_ZERO_DRAW_FROM_DENSE_GP = {17: 7.59e-9, 33: 3.10e-8, 48: 2.26e-8, 63: 5.59e-8}      # (absolute; measured on the CPU on draw_case(d))


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def build(d, T):
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)
    assert len(model["x0m"]) == d
    return model


def draw(model, seed):
    T, d = model["T"], len(model["x0m"])
    rng = np.random.default_rng(seed)
    return ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))


def white_series(model, seed):
    """white noise of the prior's marginal scale (tests/test_gpu_wide.py test_wide_logpdf_long_series_device_input): as good a series for parity as a draw"""
    return np.random.default_rng(seed).standard_normal(model["T"]) * np.sqrt(float(model["H"][0] @ model["x0P"] @ model["H"][0]) + float(model["R"][0]))


def rnew_pair(T, seed):
    return np.array([0.05]), np.random.default_rng(seed).random(T) * 0.3 + 0.01


def references(model, y, seed, dense=True):
    """what check() compares with, from the restatement and the dense GP alone: a dictionary of arrays (it travels to the child processes as an .npz)"""
    T = model["T"]
    r = dict(y=y, lp=np.float64(ref.logpdf(model, y)))
    r["fm"], r["fP"] = ref.filter_(model, y)
    post = ref.posterior(model, y)
    for tag, Rn in zip(("shared", "per_step"), rnew_pair(T, seed)):
        Rfull = np.broadcast_to(Rn, (T,))
        m_rts, v_rts = ref.marginals(ref.replace_observation_noise_cov(post, np.array(Rfull)))
        r["Rn_" + tag], r["m_rts_" + tag], r["v_rts_" + tag] = Rn, np.asarray(m_rts).reshape(T), np.asarray(v_rts).reshape(T)
        if dense:
            r["m_gp_" + tag], r["v_gp_" + tag] = dense_gp_posterior(model, y, Rfull)
    return r


def check(tgp, d, model, r, served=True, what="", post_served=None):
    """logpdf, logpdf + posterior marginals (shared and per-step Rnew) and _filter (host and device arrays) of one model against references(): the bars of
    tests/test_gpu_wide.py -- logpdf 1e-10, marginals 1e-8 (DENSE_GP_BAR) against the dense GP where the wide engine serves them (where it declines, the
    engine of before runs the reference's RTS chain and is held to the restatement alone) and 1e-6 against the literal RTS chain, _filter 1e-8 -- and
    the kernel names of the form (served = False: the engine declines, no k_wide* kernel runs, the values hold all the same; post_served: the same for the
    posterior alone, whose plan needs n1 + 1 steps behind the head for the variances of the series' end)"""
    import torch
    y, lp_ref, F = r["y"], float(r["lp"]), form_label(d)
    dm = device_model(tgp, model)
    post_served = served if post_served is None else post_served

    def named(names, label, served=served):
        if served:
            assert names == {label}, (d, what, names, label)
        else:
            assert names and not any("k_wide" in n for n in names), (d, what, names)
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, y))
    print(f"d {d} T {model['T']} {what}: logpdf {abs(lp - lp_ref) / abs(lp_ref):.2e}")
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, what, lp, lp_ref)
    named(names, F)
    for tag in ("shared", "per_step"):
        Rn = r["Rn_" + tag]
        (lp, mean, var), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, y, Rn))
        assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, what, tag, lp, lp_ref)
        named(names, F + " + k_wide_bwd", post_served)
        m_rts, v_rts = r["m_rts_" + tag], r["v_rts_" + tag]
        em, ev = np.max(np.abs(mean - m_rts)) / max(1.0, np.abs(m_rts).max()), np.max(np.abs(var - v_rts)) / max(1.0, v_rts.max())
        print(f"    {tag}: marginals vs RTS {em:.2e} {ev:.2e}")
        assert em <= 1e-6 and ev <= 1e-6, (d, what, tag, em, ev)
        if "m_gp_" + tag in r and post_served:      # (declined: the engine of before runs the reference's RTS chain -- not the code under test here; its bar is the 1e-6 above)
            m_gp, v_gp = r["m_gp_" + tag], r["v_gp_" + tag]
            em, ev = np.max(np.abs(mean - m_gp)) / max(1.0, np.abs(m_gp).max()), np.max(np.abs(var - v_gp)) / max(1.0, v_gp.max())
            print(f"    {tag}: marginals vs dense GP {em:.2e} {ev:.2e}")
            assert em <= DENSE_GP_BAR[d] and ev <= DENSE_GP_BAR[d], (d, what, tag, em, ev)
    fm_ref, fP_ref = r["fm"], r["fP"]
    for yy in (y, torch.from_numpy(np.ascontiguousarray(y)).cuda()):
        (fm, fP), names = kernels_of(tgp, dm, lambda: tgp._filter(dm, yy))
        fm, fP = (fm.cpu().numpy(), fP.cpu().numpy()) if hasattr(fm, "cpu") else (fm, fP)
        em, eP = np.max(np.abs(fm - fm_ref)) / max(1.0, np.abs(fm_ref).max()), np.max(np.abs(fP - fP_ref)) / max(1.0, np.abs(fP_ref).max())
        print(f"    _filter {em:.2e} {eP:.2e}")
        assert em <= 1e-8 and eP <= 1e-8, (d, what, em, eP)
        named(names, F + " + k_wide_fill_cov")


# --------------------------------------------------------------------------- every operation at every boundary
@pytest.mark.parametrize("d", EDGES)
def test_logpdf_posterior_marginals_and_filter_at_the_boundary_dimensions(tgp, d):
    """logpdf at 1e-10 against ref.logpdf; logpdf + posterior marginals with a shared and a per-step Rnew (1e-8 against the dense GP, 1e-6 against the literal RTS
    restatement); _filter from host and device arrays at 1e-8 against ref.filter_.  Dense-GP bar: the prototype stands within 1e-9 at every d (module docstring)."""
    T = 2500
    model = build(d, T)
    pl = wide_plan(model, T)
    assert pl["why"] == 0 and pl["chunks"] >= 4, pl
    check(tgp, d, model, references(model, draw(model, d + T), d))


@pytest.mark.parametrize("d", EDGES)
def test_logpdf_of_a_second_length_at_the_boundary_dimensions(tgp, d):
    """another length and series (T = 3000: another chunk count and last-chunk length than T = 2500), the model's handle called twice"""
    T = 3000
    model = build(d, T)
    dm = device_model(tgp, model)
    for seed in (1, 2):
        y = draw(model, 10 * d + seed)
        lp_ref = ref.logpdf(model, y)
        lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, y))
        assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, seed, lp, lp_ref)
        assert names == {form_label(d)}, names


@pytest.mark.parametrize("d", EDGES)
def test_rand_with_the_draws_supplied_at_the_boundary_dimensions(tgp, d):
    """k_wide_rand (<32> at d <= 31, <64> above: the observer lane at 48 or above from d = 48) against ref.rand on the same draws at 1e-9"""
    rng = np.random.default_rng(7 * d)
    T = 3000
    model = build(d, T)
    eps = (rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    y_ref = ref.rand(model, *eps)
    dm = device_model(tgp, model)
    y, names = kernels_of(tgp, dm, lambda: tgp.rand(eps, dm))
    err = np.max(np.abs(y - y_ref)) / max(1.0, np.abs(y_ref).max())
    print(f"d {d}: rand {err:.2e}")
    assert err <= 1e-9, (d, err)
    assert names == {"k_wide_rand"}, names


@pytest.mark.parametrize("d", EDGES)
def test_a_mean_function_at_the_inputs_at_the_boundary_dimensions(tgp, d):
    """an emission offset per step: logpdf against the restatement, posterior marginals against the dense GP on y - h (mean + h)"""
    T = 2500
    model = build(d, T)
    ht = 0.8 * np.sin(0.013 * np.arange(T)) + 0.0004 * np.arange(T) - 0.5
    y = draw(model, d) + ht
    model_h = dict(model, h=ht)
    lp_ref = ref.logpdf(model_h, y)
    dm = device_model(tgp, model_h)
    for Rn in rnew_pair(T, 100 + d):
        m_gp, v_gp = dense_gp_posterior(model, y - ht, np.broadcast_to(Rn, (T,)))
        (lp, mean, var), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, y, Rn))
        assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, lp, lp_ref)
        em, ev = np.max(np.abs(mean - (m_gp + ht))) / max(1.0, np.abs(m_gp).max()), np.max(np.abs(var - v_gp)) / max(1.0, v_gp.max())
        print(f"d {d}: with a mean function, marginals vs dense GP {em:.2e} {ev:.2e}")
        assert em <= DENSE_GP_BAR[d] and ev <= DENSE_GP_BAR[d], (d, em, ev)
        assert names == {form_label(d) + " + k_wide_bwd"}, names
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, y))
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref) and names == {form_label(d)}, (lp, lp_ref, names)


_draw_cases = {}


def draw_case(d):
    """spacing 0.1, noise 0.1, T = 3000: a series drawn from the model, then the draws of the posterior sample -- one generator, seed d (tests/test_gpu_wide_draw.py)"""
    if d not in _draw_cases:
        T = 3000
        model = build(d, T)
        rng = np.random.default_rng(d)
        y = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
        eps = (rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
        _draw_cases[d] = (model, y, eps)
    return _draw_cases[d]


def draw_c(tgp, dm, y, Rn, eps):
    """tgp_posterior_rand through ctypes on host arrays: (return code, path)"""
    hd = dm.handle()
    L = tgp._lib
    c = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64))      # noqa: E731
    yy, Rr, et, ee, e0 = c(y), c(Rn), c(eps[0]), c(eps[1]), c(eps[2])
    out = np.zeros(len(yy))
    flags = L.SHARED_R if Rr.shape[0] == 1 else 0
    rc = hd.lib.tgp_posterior_rand(hd.h, L.ptr(yy), L.ptr(Rr), L.ptr(et), L.ptr(ee), L.ptr(e0), flags, L.ptr(out))
    return rc, out


@pytest.mark.parametrize("d", sorted(REL_DRAW_RESTATEMENT))
def test_the_posterior_draw_at_the_boundary_dimensions(tgp, d):
    """tgp_posterior_rand: the same draws against ref.posterior + ref.rand relative to the path's largest value (REL_DRAW_RESTATEMENT: the module docstring has the
    measurement behind d = 17); all draws zero against the dense GP's posterior mean at ten times the oracle's own distance from it"""
    model, y, eps = draw_case(d)
    T = model["T"]
    Rn = np.array([1e-6])
    dm = device_model(tgp, model)
    (rc, got), names = kernels_of(tgp, dm, lambda: draw_c(tgp, dm, y, Rn, eps))
    assert rc == 0, rc
    assert names == {"k_wide_post_rand: " + form_label(d) + " + k_wide_post_rand"}, names
    want = ref.rand(ref.replace_observation_noise_cov(ref.posterior(model, y), Rn), *eps)
    err = np.max(np.abs(got - want)) / np.abs(want).max()
    print(f"d {d}: draw vs restatement {err:.3e} (bound {REL_DRAW_RESTATEMENT[d]:.0e})")
    assert err <= REL_DRAW_RESTATEMENT[d], (d, err)
    zero = (np.zeros((T, d)), np.zeros(T), np.zeros(d))
    rcz, path0 = draw_c(tgp, dm, y, Rn, zero)
    assert rcz == 0
    m_gp, _ = dense_gp_posterior(model, y, np.zeros(T))
    ez = np.max(np.abs(path0 - m_gp))
    print(f"d {d}: zero draw vs dense GP {ez:.3e} (oracle's own: {ORACLE_ZERO_DRAW_FROM_DENSE_GP[d]:.2e})")
    assert ez <= 10.0 * ORACLE_ZERO_DRAW_FROM_DENSE_GP[d], (d, ez)


# --------------------------------------------------------------------------- chunk geometry: small lengths
@pytest.mark.parametrize("d", GEOMETRY_D)
def test_small_lengths_behind_the_head(tgp, d):
    """T = n0 + k: declined at k = 63 (no k_wide* kernel, the values hold), one chunk of exactly 64 steps, the first partial 16-block (65), 79 / 80 (a full fifth
    16-block or not), 127 / 128 / 129 and 3 * 64 + 1 (whole 64-step blocks and one step more; still one chunk at these halos -- module docstring), and the first
    length of two chunks.  Geometry asserted from the plan at that very length.  logpdf and _filter are served from n0 + 64; the posterior needs n1 + 1 = 134 ... 175 steps
    behind the head for its end-of-series variances and is declined below (no k_wide* kernel, the values hold): its backward kernel runs at 3 * 64 + 1 and two chunks.
    So k_wide_bwd never sees the single 64-step chunk, the partial 16-block of 65 / 79 / 80 or the block edges of 127 ... 129: its single-chunk cases are k = 193 here
    and the forced one-chunk child of test_forced_chunk_counts alone."""
    n0, halo = (wide_plan(build(d, 3000), 3000)[k] for k in ("n0", "halo"))
    two = 2 * max(64, halo // 2) + 1
    posterior_lengths = 0
    for k in (63, 64, 65, 79, 80, 127, 128, 129, 3 * 64 + 1, two):
        T = n0 + k
        model = build(d, T)
        pl = wide_plan(model, T, post=1)
        if k == 63:
            assert pl["why"] != 0 and pl["chunks"] == 0, pl
        else:
            assert (pl["why_post"] == 0) == (k >= pl["n1"] + 1), (k, pl)      # (the posterior: n0 + n1 + 1 steps at least)
            assert pl["why"] == 0 and pl["n0"] == n0, pl
            assert (pl["chunks"] - 1) * pl["chunk_len"] < k <= pl["chunks"] * pl["chunk_len"], (k, pl)
            if k < 128:      # (fewer than two 64-step chunks' worth of steps)
                assert (pl["chunks"], pl["chunk_len"]) == (1, k), (k, pl)
            if k == two:
                assert (pl["chunks"], pl["chunk_len"]) == (2, (k + 1) // 2), (k, pl)
        check(tgp, d, model, references(model, draw(model, 1000 * d + k), k), served=k != 63, post_served=k != 63 and pl["why_post"] == 0,
              what=f"n0 + {k}: {pl['chunks']} x {pl['chunk_len']}, posterior {'served' if k != 63 and pl['why_post'] == 0 else 'declined'}")
        posterior_lengths += k != 63 and pl["why_post"] == 0
    assert posterior_lengths >= 2, posterior_lengths


def length_with_a_short_last_chunk(n0, halo):
    """a length behind the head whose plan ends in a chunk of 1 ... 15 steps, with a chunk count that is no multiple of four.  The search restates plan()'s rule
    for lengths this short; the test asserts what the plan itself reports."""
    hm = max(64, halo // 2)
    for Tb in range(64 * 64, 40 * hm * hm):
        c0 = max(1, min(4096, Tb // 64, Tb // hm))
        ln = -(-Tb // c0)
        c = -(-Tb // ln)
        if 1 <= Tb - (c - 1) * ln <= 15 and c % 4:
            return n0 + Tb
    raise AssertionError("no such length")


@pytest.mark.parametrize("d", GEOMETRY_D)
def test_a_last_chunk_of_a_few_steps_against_the_c_oracle(tgp, d):
    """a last chunk of 1 ... 15 steps in a wave with invalid rows, at a length (T = 16821, 16820, 23626, 26146 at d = 12, 28, 42, 54: 123, 123, 147, 155 chunks, the last of 15 steps) where the C oracle is the reference: logpdf at 1e-10, posterior marginals at
    1e-6 against its RTS chain (the project's bar against an RTS chain), _filter (d = 12, 28) at 1e-8 against its filtered states"""
    import torch
    pl0 = wide_plan(build(d, 3000), 3000)
    T = length_with_a_short_last_chunk(pl0["n0"], pl0["halo"])
    model = build(d, T)
    pl = wide_plan(model, T)
    last = (T - pl["n0"]) - (pl["chunks"] - 1) * pl["chunk_len"]
    print(f"d {d}: T {T} plan {pl} last chunk {last}")
    assert pl["why"] == 0 and 1 <= last <= 15 and pl["chunks"] % 4 != 0, (pl, last)
    y = white_series(model, d)
    lp_ref = sk.logpdf(model, y)
    dm = device_model(tgp, model)
    Rn = np.random.default_rng(d).random(T) * 0.3 + 0.01
    m_ref, v_ref = sk.posterior_marginals(model, y, Rn)
    (lp, mean, var), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, y, Rn))
    assert names == {form_label(d) + " + k_wide_bwd"}, names
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, lp, lp_ref)
    em, ev = np.max(np.abs(mean - m_ref)) / max(1.0, np.abs(m_ref).max()), np.max(np.abs(var - v_ref)) / max(1.0, v_ref.max())
    print(f"    marginals vs the oracle's RTS chain {em:.2e} {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6, (d, em, ev)
    if d > 28:      # (_filter returns T d^2 doubles of covariances: half a gigabyte and more at these lengths from d = 42)
        return
    _, fm_ref, fP_ref = sk.filter_(model, y, want_states=True)
    (fm, fP), names = kernels_of(tgp, dm, lambda: tgp._filter(dm, torch.from_numpy(y).cuda()))
    assert names == {form_label(d) + " + k_wide_fill_cov"}, names
    fm, fP = fm.cpu().numpy(), fP.cpu().numpy()
    assert np.max(np.abs(fm - fm_ref)) <= 1e-8 * max(1.0, np.abs(fm_ref).max()), np.max(np.abs(fm - fm_ref))
    assert np.max(np.abs(fP - fP_ref)) <= 1e-8 * max(1.0, np.abs(fP_ref).max()), np.max(np.abs(fP - fP_ref))


# --------------------------------------------------------------------------- chunk geometry: forced counts, the LDS family (child processes)
def child(env, code, timeout):
    """one child process at a time, its own time limit, a non-zero exit fails the test with the child's output, nothing is retried"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **env), cwd=ROOT)
    assert r.returncode == 0 and "checked" in r.stdout, (env, (r.stdout + r.stderr)[-4000:])
    return r.stdout


def child_check(path, dims, chunks=None, adjoint=False):
    """(runs in the child) check() of every d in dims on the references the parent stored; the forced chunk count asserted from the plan AND from the kernel's name"""
    import temporalgps_jl_amd as tgp
    tgp._lib.load()
    for d in dims:
        r = dict(np.load(os.path.join(path, f"ref{d}.npz")))
        T = len(r["y"])
        model = build(d, T)
        pl = wide_plan(model, T)
        assert pl["why"] == 0, pl
        if chunks is not None:
            assert pl["chunks"] == chunks and pl["chunk_len"] == -(-(T - pl["n0"]) // chunks), (chunks, pl)
        check(tgp, d, model, r, what=f"{pl['chunks']} x {pl['chunk_len']}")
        if adjoint:
            from tests.test_gpu_wide_adjoint import test_block_gradients_against_directional_differences_of_the_oracle as adjoint_test
            adjoint_test(tgp, d)
    print("checked")


@pytest.fixture(scope="module")
def stored_references(tmp_path_factory):
    """references() of the T = 3000 case of every geometry d, computed once and read by every child"""
    path = str(tmp_path_factory.mktemp("wide_edges"))
    for d in GEOMETRY_D:
        model = build(d, 3000)
        np.savez(os.path.join(path, f"ref{d}.npz"), **references(model, draw(model, 31 * d), d))
    return path


CHILD = "import sys\nsys.path.insert(0, {root!r})\nfrom tests.test_gpu_wide_edges import child_check\nchild_check({path!r}, {dims!r}, chunks={chunks!r}, adjoint={adjoint!r})\n"


@pytest.mark.parametrize("chunks", (1, 2, 3, 5, 7))
def test_forced_chunk_counts(stored_references, chunks):
    """TGP_WIDE_CHUNKS (read once per process; it can only lower the count) at T = 3000: chunks several halos long, so a warm-up from zero crosses many 16- and 64-step
    blocks, and one to three invalid rows in the last DPP wave.  The child asserts info[6] == the forced count and the parities of check()."""
    out = child({"TGP_WIDE_CHUNKS": str(chunks)}, CHILD.format(root=ROOT, path=stored_references, dims=GEOMETRY_D, chunks=chunks, adjoint=False), timeout=420)
    print(out[-3000:])


def test_the_lds_family_for_every_d(stored_references):
    """TGP_WIDE_DPP=0 (DESIGN 4.4's A/B path): k_wide_lml<32> / k_wide_bwd<32, .> at d = 12, 28 and <64> at d = 42 -- logpdf, posterior marginals, _filter and the adjoint
    (tests/test_gpu_wide_adjoint.py's directional differences, which assert the family's name too)"""
    assert [form_label(d, dpp=False) for d in (12, 28, 42)] == ["k_wide_lml<32>", "k_wide_lml<32>", "k_wide_lml<64>"]
    out = child({"TGP_WIDE_DPP": "0"}, CHILD.format(root=ROOT, path=stored_references, dims=(12, 28, 42), chunks=None, adjoint=True), timeout=600)
    print(out[-3000:])      # (the child's check() and adjoint test assert the <32> / <64> labels: form_label reads the same variable)


# --------------------------------------------------------------------------- chunk geometry: long series against the C oracle
def long_case(tgp, d, T):
    import torch
    model = build(d, T)
    y = white_series(model, d)
    return model, y, torch.from_numpy(y).cuda(), device_model(tgp, model)


@pytest.mark.parametrize("d", (9, 12))
def test_more_than_4096_chunks_against_the_c_oracle(tgp, d):
    """the regime of want = Tb / (4 halo) chunks (the one behind the README's T = 1e7 numbers): about 4195 chunks of four halos and a step, the last one shorter (T = 2.6e6
    and 4.6e6) -- device arrays, logpdf at 1e-10 against the C oracle, posterior marginals at 1e-6 against its RTS chain.  (The oracle's two passes take 25 s at d = 9
    and 75 s at d = 12 on one core.)"""
    pl0 = wide_plan(build(d, 3000), 3000)
    T = pl0["n0"] + 4 * pl0["halo"] * 4200 - 5
    model, y, yd, dm = long_case(tgp, d, T)
    pl = wide_plan(model, T)
    print(f"d {d}: T {T} plan {pl}")
    assert pl["why"] == 0 and pl["chunks"] > 4096 and pl["chunk_len"] >= 4 * pl["halo"], pl
    lp_ref = sk.logpdf(model, y)
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, yd))
    print(f"    logpdf {abs(lp - lp_ref) / abs(lp_ref):.2e}")
    assert names == {form_label(d)}, names
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, lp, lp_ref)
    import torch
    Rn = np.array([0.2])
    m_ref, v_ref = sk.posterior_marginals(model, y, Rn)
    (mean, var), names = kernels_of(tgp, dm, lambda: tgp.posterior_marginals(dm, yd, torch.from_numpy(Rn).cuda()))
    assert names == {form_label(d) + " + k_wide_bwd"}, names
    mean, var = mean.cpu().numpy(), var.cpu().numpy()
    em, ev = np.max(np.abs(mean - m_ref)) / max(1.0, np.abs(m_ref).max()), np.max(np.abs(var - v_ref)) / max(1.0, v_ref.max())
    print(f"    marginals vs the oracle's RTS chain {em:.2e} {ev:.2e}")
    assert em <= 1e-6 and ev <= 1e-6, (d, em, ev)


@pytest.mark.parametrize("d", (33, 54))
def test_exactly_4096_chunks_longer_than_their_warm_up_against_the_c_oracle(tgp, d):
    """4096 chunks of halo + 1 steps, the last one five steps short (T = 1.4e6: the shortest series of this geometry -- the oracle's filter takes 40 s at d = 33 and two
    and a half minutes at d = 54 on one core): device arrays, logpdf at 1e-10 against the C oracle"""
    pl0 = wide_plan(build(d, 3000), 3000)
    T = pl0["n0"] + 4096 * (pl0["halo"] + 1) - 5
    model, y, yd, dm = long_case(tgp, d, T)
    pl = wide_plan(model, T)
    print(f"d {d}: T {T} plan {pl}")
    assert pl["why"] == 0 and pl["chunks"] == 4096 and pl["chunk_len"] > pl["halo"], pl
    lp_ref = sk.logpdf(model, y)
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, yd))
    print(f"    logpdf {abs(lp - lp_ref) / abs(lp_ref):.2e}")
    assert names == {form_label(d)}, names
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, lp, lp_ref)
