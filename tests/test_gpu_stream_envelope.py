"""GPU tier: the streaming kernels (csrc/tgp_lml.hip k_lml_stream, csrc/tgp_post.hip k_post_stream) and their fall-back k_steady_one across the envelope the
host plan serves them in -- the case table of tests/_stream_envelope.py, placed on the plan by tests/test_stream_envelope_host.py: halos from the smallest
to the cap and past it, either side of the posterior kernel's halo <= tile and of the d = 1 logpdf kernel's switch to the 2048-step tile, the longest and
the shortest heads, eigenvector conditioning up to kCondMax and past it, input coefficients down to kRelMin and below it, noise from 1e-6 to 1e3 of the
signal, offsets thousands of standard deviations from zero.  Through the C ABI with TGP_OPT_STREAM_MIN_T = 0 on the handle, against the oracle's
sequential filter / smoother in double (oracle/seq_kalman.c) at the project's bars -- logpdf 1e-10 relative, mean and var 1e-8 max(1, scale) -- and
every call asserts the set of kernels that served it.

Lengths per case from its own head, halo and tile: nhs + 2, nhs + halo -+ 1, nhs + tile + 1, nhs + 2 tile + 37, nhs + 3 tile.  Who serves them follows
from the host code (restated in tests/_stream_envelope.py server(), asserted against the sources on the CPU tier): a logpdf call goes to k_lml_stream at
every length the plan's core accepts (unless the form's closure amplification exceeds kClosureAmpMax: then to k_steady_one, as below kRelMin); a posterior call goes to k_post_stream only with the head on the host, which tgp_modal.hip plan() arranges from
T >= nhs + kTailMax + 1 on -- the two longest lengths -- and below that to k_steady_one, or, where the series is shorter than head + variance transient
(build_tables_tail: nhs + n1 + 1 > T), to neither.

Every line printed with the prefix ENVELOPE is a row of profiles/stream_envelope_parity.txt."""
import numpy as np
import pytest

from tests import _stream_envelope as E
from tests.test_gpu_stream_form import device_model, kernels_of

pytestmark = pytest.mark.gpu

NAMES = [c["name"] for c in E.CASES]
POSTERIOR = [c["name"] for c in E.CASES if len(E.model_of(c, 4)["x0m"]) <= 3]
FAMILIES = ("k_lml_stream", "k_post_stream", "k_steady_one")


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def assert_server(names, want, what):
    if want in (E.LML16, E.LML32, E.POST):
        assert names == {want}, (what, want, names)
    elif want == E.STEADY:
        assert len(names) == 1 and next(iter(names)).startswith("k_steady_one"), (what, want, names)
    else:      # declined by the plan on the host, before any launch: another engine serves
        assert names and not any(n.startswith(f) for n in names for f in FAMILIES), (what, want, names)


def plan_columns(pl):
    if pl["why"] != E.OK:
        return f"why {pl['why']} n0 {pl['n0']} cond_f {pl['cond_f']:.3e} cond_g {pl['cond_g']:.3e}"
    return (f"halo {pl['halo']} n0 {pl['n0']} nhs {pl['nhs']} npair {pl['npair']} cond_f {pl['cond_f']:.3e} cond_g {pl['cond_g']:.3e} "
            f"ratio {E.form_ratio(pl):.3e}")


def deviations(mean, var, m_ref, v_ref):
    return (float(np.max(np.abs(mean - m_ref)) / max(1.0, np.max(np.abs(m_ref)))), float(np.max(np.abs(var - v_ref)) / max(1.0, np.max(np.abs(v_ref)))))


def run_logpdf(tgp, name, T):
    pl = E.plan_of(E.BY_NAME[name])
    model, y = E.series(name, T)
    lp_ref = E.reference(name, T, posterior=False)[0]
    dm = device_model(tgp, model)
    lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, y))
    rel = abs(lp - lp_ref) / abs(lp_ref)
    print(f"ENVELOPE {name} T {T} logpdf {plan_columns(pl)} served {'+'.join(sorted(names))} logpdf_rel {rel:.2e}")
    assert_server(names, E.server(pl, T, False), (name, T, "logpdf"))
    assert rel <= E.LP_BAR, (name, T, lp, lp_ref)
    return names


def run_posterior(tgp, name, T, per_step):
    pl = E.plan_of(E.BY_NAME[name])
    model, y = E.series(name, T)
    lp_ref, m_ref, v_ref, v_ref_t = E.reference(name, T)
    Rn = E.rnew_per_step(T) if per_step else E.RN
    dm = device_model(tgp, model)
    (lp, mean, var), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, y, Rn))
    rel = abs(lp - lp_ref) / abs(lp_ref)
    dm_, dv_ = deviations(mean, var, m_ref, v_ref_t if per_step else v_ref)
    print(f"ENVELOPE {name} T {T} posterior{'/step' if per_step else ''} {plan_columns(pl)} served {'+'.join(sorted(names))} "
          f"logpdf_rel {rel:.2e} mean_dev {dm_:.2e} var_dev {dv_:.2e}")
    assert_server(names, E.server(pl, T, True), (name, T, "posterior"))
    assert rel <= E.LP_BAR and dm_ <= E.MV_BAR and dv_ <= E.MV_BAR, (name, T, rel, dm_, dv_)
    return names


# ------------------------------------------------------------------------------------------------------------ 1. values and who served
@pytest.mark.parametrize("name", NAMES)
def test_logpdf_over_the_envelope(tgp, name):
    c = E.BY_NAME[name]
    for T in E.case_lengths(c, False) if c["why"] == E.OK else E.declined_lengths(c):
        run_logpdf(tgp, name, T)


@pytest.mark.parametrize("name", POSTERIOR)
def test_posterior_over_the_envelope(tgp, name):
    """with one new noise variance for the series and with one per step"""
    c = E.BY_NAME[name]
    for T in E.case_lengths(c, True) if c["why"] == E.OK else E.declined_lengths(c):
        for per_step in (False, True):
            run_posterior(tgp, name, T, per_step)


# ------------------------------------------------------------------------------------------------------------ 2. either side of each threshold
@pytest.mark.parametrize("inside,beyond", E.PAIRS)
def test_both_sides_of_a_threshold_agree_with_the_oracle_each_on_its_own_server(tgp, inside, beyond):
    """the two models of a pair differ by half a percent of the spacing (or of the stretch, or a factor two in a faint variance): each at the bars on its
    own server, and the servers differ where the guard says so -- this pins the <= / < of each guard"""
    pa, pb = E.plan_of(E.BY_NAME[inside]), E.plan_of(E.BY_NAME[beyond])
    T = E.all_lengths(E.BY_NAME[inside])[-1]
    la, lb = run_logpdf(tgp, inside, T), run_logpdf(tgp, beyond, T)
    served = lambda names, fam: all(n.startswith(fam) for n in names)
    if inside.endswith("_1024"):
        assert la == {E.LML16 if pa["d"] == 1 else E.LML32} and lb == {E.LML32}      # (the d = 1 tile switch: 64 * 16 < halo)
    else:
        assert served(la, "k_lml_stream") and not served(lb, "k_lml_stream"), (la, lb)
        assert served(lb, "k_steady_one") == (beyond in ("relmin_below", "amp_beyond")), lb
    if pa["d"] <= 3:
        qa, qb = run_posterior(tgp, inside, T, False), run_posterior(tgp, beyond, T, False)
        if inside.endswith("_cap"):
            assert served(qa, "k_steady_one") and not any(n.startswith(f) for n in qb for f in FAMILIES), (qa, qb)
        elif inside == "amp_in":      # (the closure is the logpdf kernel's alone)
            assert qa == qb == {E.POST}, (qa, qb)
        else:
            assert qa == {E.POST} and served(qb, "k_steady_one"), (qa, qb)
    assert pb["why"] != E.OK or pb["nhs"] + 2 <= T


# ------------------------------------------------------------------------------------------------------------ 3. the inputs are read
def test_a_bump_a_quarter_tile_in_front_of_a_seam_is_followed(tgp):
    """the mutation: on the halo-1024 case at d = 1 (of the four, the one whose series stays nearest zero: 1e-3 times the smoother's weight at the bump,
    0.022, is 1.7e-5 of its scale in the oracle, 8e-6 .. 1.2e-5 for the others), head + three tiles (every tile a run of its own: seams at the tile edges), y moves by 1e-3 at 256 steps
    in front of the last seam.  The device follows the oracle of the bumped series on both sides of the seam, and the oracle of the series as it
    was then misses the mean's bar a thousandfold"""
    name = "halo_d1_1024"
    pl = E.plan_of(E.BY_NAME[name])
    T = pl["nhs"] + 3 * E.K_TILE_POST
    seam = pl["nhs"] + 2 * E.K_TILE_POST
    model, y = E.series(name, T)
    _, m_old, v_old, _ = E.reference(name, T)
    from oracle import seq_kalman as sk
    bumped = np.array(y)
    bumped[seam - 256] += 1e-3
    m_ref, v_ref = sk.posterior_marginals(model, bumped, E.RN)
    lp_ref = sk.logpdf(model, bumped)
    dm = device_model(tgp, model)
    (lp, mean, var), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, bumped, E.RN))
    assert names == {E.POST}, names
    scale = max(1.0, np.max(np.abs(m_ref)))
    left, right = np.max(np.abs(mean - m_ref)[:seam]) / scale, np.max(np.abs(mean - m_ref)[seam:]) / scale
    miss = np.max(np.abs(mean - m_old)) / scale
    print(f"ENVELOPE-BUMP {name} T {T} seam {seam}: mean_dev left {left:.2e} right {right:.2e}, against the series as it was {miss:.2e}, logpdf_rel {abs(lp - lp_ref) / abs(lp_ref):.2e}")
    assert left <= E.MV_BAR and right <= E.MV_BAR and abs(lp - lp_ref) <= E.LP_BAR * abs(lp_ref)
    assert np.max(np.abs(var - v_ref)) <= E.MV_BAR
    assert miss >= 1e3 * E.MV_BAR, miss


# ------------------------------------------------------------------------------------------------------------ 4. device pointers, repeats
def test_device_resident_series_and_outputs_and_repeats_around_another_model(tgp):
    """a long-halo case with y, the new noise variances and both outputs in device memory; the same call twice on one handle is bit-identical, with
    another model of the same state dimension planned in between (the form is kept with the plan's core, and the stages behind the core read a
    per-thread workspace)"""
    import torch
    name, other = "halo_d3_1024", "noise_10"
    pl = E.plan_of(E.BY_NAME[name])
    T = pl["nhs"] + 2 * E.K_TILE_POST + 37
    model, y = E.series(name, T)
    lp_ref, m_ref, v_ref, _ = E.reference(name, T)
    dm = device_model(tgp, model)
    yd, rd = torch.from_numpy(np.array(y)).cuda(), torch.from_numpy(E.RN.copy()).cuda()
    To = E.case_lengths(E.BY_NAME[other], True)[-1]
    mo, yo = E.series(other, To)
    lpo_ref, mo_ref, vo_ref, _ = E.reference(other, To)
    dmo = device_model(tgp, mo)
    got = []
    for rep in range(2):
        bm, bv = torch.zeros(T, dtype=torch.float64, device="cuda"), torch.zeros(T, dtype=torch.float64, device="cuda")
        lp, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, yd))
        assert names == {E.LML32}, names
        (mean, var), names = kernels_of(tgp, dm, lambda: tgp.posterior_marginals(dm, yd, rd, out=(bm, bv)))
        assert names == {E.POST}, names
        mean, var = mean.cpu().numpy(), var.cpu().numpy()
        dm_, dv_ = deviations(mean, var, m_ref, v_ref)
        print(f"ENVELOPE-DEVICE {name} T {T} call {rep}: logpdf_rel {abs(lp - lp_ref) / abs(lp_ref):.2e} mean_dev {dm_:.2e} var_dev {dv_:.2e}")
        assert abs(lp - lp_ref) <= E.LP_BAR * abs(lp_ref) and dm_ <= E.MV_BAR and dv_ <= E.MV_BAR
        got.append((lp, mean, var))
        if rep == 0:
            lpo = tgp.logpdf(dmo, yo)
            _, meano, varo = tgp.logpdf_and_posterior_marginals(dmo, yo, E.RN)
            assert abs(lpo - lpo_ref) <= E.LP_BAR * abs(lpo_ref) and max(deviations(meano, varo, mo_ref, vo_ref)) <= E.MV_BAR
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])
