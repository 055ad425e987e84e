"""CPU tier: the tile sweep's algorithm (tgp_sweep_tile.hip) restated in NumPy (tests/_sweep_tile.py run_tile_sweep) on the GPU tier's
models, against the oracle at the project's bars (logpdf 1e-10 relative, marginals 1e-8 of max(1, .)) -- so that a wrong formula is not debugged on
the GPU -- and each hand-over distance a factor 10 inside kTol = 1e-12 / kTolBack = 1e-11 at the geometries the GPU tier expects to be served at the
first attempt: the forced one (C = 64, W = 128, Wb = 64 at d = 9) and the plan's own (W, Wb, C = Wb from the forgetting estimate at noise 0.1).

Measured here (mean / variance distance from the oracle's jittered RTS chain, relative to max(1, .); forward / backward hand-over distance):
  d =  9, T = 2053, forced 64 / 128 / 64:   2.6e-10 / 1.4e-10;  3.2e-16 / 2.2e-15
  d = 12, T = 2048, plan 104 / 112 / 104:   1.8e-09 / 1.2e-09;  4.3e-16 / 7.0e-16
  d = 13, T = 2053, plan 120 / 136 / 120:   1.5e-10 / 2.1e-10;  5.6e-16 / 2.7e-15   (noise and offset per step)
  d = 16, T = 2048, plan 144 / 152 / 144:   9.4e-10 / 6.3e-10;  5.6e-16 / 4.0e-15   (the oracle's own 1e-10 jitter, not rounding: all below 3e-9)"""
import numpy as np
import pytest

from tests import _sweep_tile as ST

# (d, T, xs, C, W, Wb)
CASES = [(9, 2053, 0, 64, 128, 64), (12, 2048, 0, 104, 112, 104), (13, 2053, 3, 120, 136, 120), (16, 2048, 0, 144, 152, 144)]


@pytest.mark.parametrize("d,T,xs,C,W,Wb", CASES)
def test_tile_algorithm_equals_the_oracle_and_its_hand_overs_hold(d, T, xs, C, W, Wb):
    model, y, missing, Rn, (lp, pm, pv) = ST.case(d, T, xs, True, xs != 0)
    lml, mean, var, dist = ST.run_tile_sweep(model, y, missing, Rn, C, W, Wb)
    em, ev = np.abs(mean - pm).max() / max(1.0, np.abs(pm).max()), np.abs(var - pv).max() / max(1.0, pv.max())
    print(d, T, abs(lml - lp) / abs(lp), em, ev, dist)
    assert abs(lml - lp) <= 1e-10 * abs(lp)
    assert em <= 3e-9 and ev <= 3e-9      # (the bar is 1e-8: a case beyond 3e-9 is replaced, not the bar)
    assert dist[0] <= 1e-13 and dist[1] <= 1e-12, dist


def test_the_hand_over_checks_see_warm_ups_that_are_too_short():
    model, y, missing, Rn, _ = ST.case(9, 2053)
    _, _, _, dist = ST.run_tile_sweep(model, y, missing, Rn, 64, 16, 32)
    assert dist[0] > 1e-12 and dist[1] > 1e-11, dist      # where the kernel reports bits 1 and 2
