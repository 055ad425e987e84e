"""CPU tier: the algorithm of the dense engine's passes across the chip (csrc/tgp_dense_chunked.hpp) in its NumPy restatement, scripts/dense_chunk_proto.py --
chunks behind warm-ups from x0, Bryson-Frazier backward chunks from zero adjoints, checked hand-overs, doubling, decline -- against the sequential forms of
oracle/lgssm_ref.py; and the geometries tests/test_gpu_dense_chunked.py forces: the restatement alone passes both checks there with no repair, so the GPU
tests may demand "served, one attempt each way" of the device."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def proto():
    spec = importlib.util.spec_from_file_location("dense_chunk_proto", os.path.join(ROOT, "scripts", "dense_chunk_proto.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("d", (18, 28, 42, 54))
def test_forced_geometries_pass_both_checks_without_repair_and_match_the_sequential_forms(proto, d):
    model, (C, W, Wb) = proto.test_model(d)
    assert len(model["x0m"]) == d and W <= 128 and Wb <= 128 and model["T"] % C != 0
    Rn = np.array([0.05])
    for per_step in (False, True):
        mdl, y, missing = proto.test_series(model, d, per_step_noise=per_step)
        r = proto.run(mdl, y, missing, Rn, C, W, Wb)
        print(d, per_step, r["dist_f"], r["dist_b"])
        assert r["served"] == 1 and r["attempts"] == 2 and r["chunks"] > 1, r      # (one forward and one backward round)
        assert r["dist_f"] <= proto.TOL_F and r["dist_b"] <= proto.TOL_B
        if per_step:
            continue
        lp = ref.logpdf_missing(mdl, y, missing)
        assert abs(r["lml"] - lp) <= 1e-10 * abs(lp), (r["lml"], lp)
        m_bf, v_bf = ref.bryson_frazier_marginals(mdl, y, Rn, missing=missing)
        assert np.max(np.abs(r["mean"] - m_bf)) <= 1e-8 * max(1.0, np.abs(m_bf).max())
        assert np.max(np.abs(r["var"] - v_bf)) <= 1e-8 * max(1.0, v_bf.max())


def _slow_model(proto, T):
    """A long length scale observed almost without noise: the prior remembers a state for hundreds of steps, the filter for about a hundred observed ones
    (W = 128 passes the check, 64 does not).  The algorithm does not depend on d: d = 3 keeps these cases quick."""
    return oc.build_lgssm(("stretched", 0.05, ("matern52",)), ("regular", 0.0, 0.2, T), 1e-6)


def test_a_missing_stretch_longer_than_a_forced_warm_up_fails_the_forward_check(proto):
    """Over missing steps the filter does not forget at the closed loop's rate but at the prior's: a warm-up that lies inside the stretch hands over a state
    that still remembers x0.  The check must say so; a forced geometry is then declined, not repaired."""
    T, C, W = 1500, 300, 128
    mdl, y, missing = proto.test_series(_slow_model(proto, T), 1, frac_missing=0.0)
    missing[2 * C - 148:2 * C] = True           # the 148 steps in front of chunk 2
    r = proto.run(mdl, y, missing, None, C, W, 0)
    assert r["served"] == 0 and r["status"] == 1 and r["attempts"] == 1 and r["dist_f"] > proto.TOL_F, r
    clear = proto.run(mdl, y, np.zeros(T, dtype=bool), None, C, W, 0)
    assert clear["served"] == 1 and clear["dist_f"] <= proto.TOL_F, clear


def test_automatic_geometry_doubles_the_warm_up_and_declines_beyond_half_a_chunk(proto):
    T = 4096
    mdl, y, missing = proto.test_series(_slow_model(proto, T), 2, frac_missing=0.0)
    missing[964:1030] = True                     # across the boundary at 1024: the first warm-up sees 68 observed steps only
    r = proto.run(mdl, y, missing, np.array([0.05]), guess=128)      # chunks of 4 x 128 steps
    lp = ref.logpdf_missing(mdl, y, missing)
    assert r["served"] == 1 and r["attempts"] > 2 and r["W"] > 128, r
    assert abs(r["lml"] - lp) <= 1e-10 * abs(lp)
    m_bf, v_bf = ref.bryson_frazier_marginals(mdl, y, np.array([0.05]), missing=missing)
    assert np.max(np.abs(r["mean"] - m_bf)) <= 1e-8 * max(1.0, np.abs(m_bf).max()) and np.max(np.abs(r["var"] - v_bf)) <= 1e-8 * max(1.0, v_bf.max())
    missing[700:1030] = True                    # longer than any warm-up that leaves C >= 2 W
    r = proto.run(mdl, y, missing, None, guess=128)
    assert r["served"] == 0 and r["status"] == 1 and r["attempts"] >= 2, r
    short = proto.run(dict(mdl, T=3000), y[:3000], missing[:3000], None, guess=128)     # fewer than 8 chunks of 4 W: never tried
    assert short["served"] == 0 and short["attempts"] == 0
