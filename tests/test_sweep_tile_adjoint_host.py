"""CPU tier: the chunked walk of k_sweep_tile_adjoint (tgp_sweep_tile.hip) restated in NumPy (tests/_sweep_tile_adjoint.py run_tile_adjoint) on the
GPU tier's four parity cases against the long-double recursion (tests/_sweep_adjoint.py restated) at that tier's bars -- logpdf 1e-10 relative, every
gradient entry 1e-8 of its block's largest, both hand-over distances inside kTol = 1e-12 / kTolBack = 1e-11 -- so that a wrong formula or hand-over is not
debugged on the GPU."""
import pytest

from tests import _sweep_adjoint as SA
from tests import _sweep_tile_adjoint as TA


@pytest.mark.parametrize("d,T,xs,C,W,Wa", TA.CASES)
def test_the_chunked_walk_equals_the_recursion_and_its_hand_overs_hold(d, T, xs, C, W, Wa):
    model, y, missing, lp, want = TA.case(d, T, xs)
    lml, g, dist = TA.run_tile_adjoint(model, y, missing, C, W, Wa)
    dev = SA.block_deviations(g, want, SA.BLOCKS + ("h_steps", "R_steps"))
    print(d, T, abs(lml - lp) / abs(lp), dev, dist)
    assert abs(lml - lp) <= SA.LP_BAR * abs(lp)
    assert max(dev.values()) <= SA.GRAD_BAR, dev
    assert dist[0] <= 1e-12 and dist[1] <= 1e-11, dist


def test_the_backward_check_sees_a_warm_up_of_16_steps():
    model, y, missing, _, _ = TA.case(9, 2053, 0)
    _, _, dist = TA.run_tile_adjoint(model, y, missing, 64, 128, 16)
    assert dist[0] <= 1e-12 < 1e-11 < dist[1], dist      # where the kernel reports bit 2
