"""CPU tier: the ALGORITHM of the wide-state engine's posterior draw (scripts/wide_draw_proto.py: the draw plan, chunks that start halo_draw steps late
from zero on the same streams, the head on the host -- csrc/tgp_wide.hip's plan_draw and k_wide_post_rand restated in NumPy) against the oracle's literal
restatement: rand (lgssm.jl:65-91) of the Reverse model posterior (lgssm.jl:193-238) builds, on the same draws.  This pins that the recursion in the
deviation from the filtered mean IS the reference's draw and that chunking with a halo is exact, separately from any kernel.  The HIP kernel:
tests/test_gpu_wide_draw.py; the product's own host plan: tests/test_wide_draw_plan.py.

Bounds (relative to the path's largest value), a priori: both sides evaluate the same recursion in double precision and differ by rounding alone, which the
solve against the predicted covariance amplifies by its condition number -- 2e4 at d = 9 (1e-9, the bar of tgp_rand, leaves three decades), 2.9e8 at
d = 28 (1e-6, the project's bar against the literal RTS chain at that d).  Measured at T = 3000, five chunks: 6.2e-13 (d = 9), 4.1e-15 (d = 28)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {
    9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))),
    28: ("product", ("approx_periodic", 7, 1.0), ("matern32",)),
}
BOUND = {9: 1e-9, 28: 1e-6}


def _load(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


@pytest.fixture(scope="module")
def protos():
    return _load("wide_proto"), _load("wide_draw_proto")


@pytest.mark.parametrize("per_step_noise", (False, True))
@pytest.mark.parametrize("d", sorted(KERNELS))
def test_chunked_draw_in_the_deviation_from_the_filtered_mean_equals_the_oracle(protos, d, per_step_noise):
    wp, dp = protos
    T, chunks = 3000, 5
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)
    assert len(model["x0m"]) == d
    rng = np.random.default_rng(d)
    y = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    et, ee, e0 = rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d)
    Rn = rng.random(T) * 0.2 + 0.01 if per_step_noise else np.array([1e-6])
    pl = wp.plan(model, T)
    assert pl is not None
    dpl = dp.plan_draw(model, pl, dp.head_covariances(model, pl["n0"]))
    # at least three chunks start from zero, halo_draw steps behind their end
    ln = -(-(T - pl["n0"]) // chunks)
    assert dpl["halo"] is not None and sum(pl["n0"] + (c + 1) * ln + dpl["halo"] < T for c in range(chunks)) >= 3, (dpl["halo"], ln)
    out = dp.run(pl, dpl, y, Rn, et, ee, e0, chunks=chunks)
    want = ref.rand(ref.replace_observation_noise_cov(ref.posterior(model, y), Rn), et, ee, e0)
    err = np.max(np.abs(out - want)) / np.abs(want).max()
    print(f"d {d} n0 {pl['n0']} halo_draw {dpl['halo']}: prototype vs restatement {err:.3e}")
    assert err <= BOUND[d], err
    one = dp.run(pl, dpl, y, Rn, et, ee, e0, chunks=1)      # (one chunk: the plain recursion from the drawn end state)
    assert np.max(np.abs(out - one)) <= 1e-12 * np.abs(want).max()
