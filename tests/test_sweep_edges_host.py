"""CPU tier: the case table of the sweep engine's edge tests (tests/_sweep_edges.py) on the host -- the product's own plan and per-lane code
(tests/hostsim/sweepsim.cpp, sweepdrawsim.cpp) inside the repair loop of the C ABI's call (_util.sweepsim_served, _sweepdraw.sweepdrawsim_served).  Every
entry is checked for what the device tier (tests/test_gpu_sweep_edges.py) relies on:

  * the outcome the table states: served, status bits, attempts -- of the logpdf call, the posterior call and the draw;
  * the margin: in every attempt the hand-over distances lie at least a factor 10 on their side of kTol = 1e-12 / kTolBack = 1e-11, so that rounding
    differences between host and device cannot flip an outcome;
  * a served call's values at the project's bars (logpdf 1e-10 relative, marginals 1e-8 of their scale against oracle/lgssm_ref.py, the C restatement above
    6000 steps; a draw 1e-9 against the walk restated in NumPy).

`python -m tests.test_sweep_edges_host` prints every entry's geometry and distances (the table in the device tier's docstring)."""
import numpy as np
import pytest

from tests import _sweep_edges as E

NAMES = [c.name for c in E.TABLE]


def _values_at_the_bars(c, h, post):
    lp, pm, pv = E.reference(c)
    assert abs(h["lml"] - lp) <= 1e-10 * abs(lp), (h["lml"], lp)
    if post:
        assert np.abs(h["mean"] - pm).max() <= 1e-8 * max(1.0, np.abs(pm).max())
        assert np.abs(h["var"] - pv).max() <= 1e-8 * max(1.0, pv.max())


@pytest.mark.parametrize("name", NAMES)
def test_table_entry_on_the_host(name):
    c = E.BY_NAME[name]
    if c.what == "draw":
        h = E.host(c)
        tries = h.get("tries") or [(h["C"], h["W"], h["Wd"], h["status"], float(h["dist_f"]), float(h["dist_d"]))]
        print(name, "draw", tries)
        assert h["rc"] == 0 and (h["served"], h["status"], h["attempts"]) == c.draw, (h["status"], h["attempts"], tries)
        assert h["status"] & 12 or E.margins_hold(tries), tries
        if h["served"]:
            want = E.draw_reference(c)
            assert np.abs(h["y"] - want).max() <= 1e-9 * max(1.0, np.abs(want).max())
        return
    for post, want in ((False, c.lp), (True, c.post)):
        if want is None:
            continue
        h = E.host(c, post)
        print(name, "posterior" if post else "logpdf", h["why"], h["tries"])
        assert (h["served"], h["status"], h["attempts"]) == want, (h["served"], h["status"], h["attempts"], h["why"], h["tries"])
        assert h["status"] & 12 or E.margins_hold(h["tries"], post), h["tries"]
        if c.force:      # a forced geometry is reported as it was asked for (Wb never above C)
            assert h["tries"][0][:3] == (c.force[0], c.force[1], min(c.force[2], c.force[0])), h["tries"]
        if h["served"]:
            _values_at_the_bars(c, h, post)


def test_the_ties_sit_where_the_table_says():
    """group D: step 1, the last step, sixteen steps in a row from step 800 and the first steps of the second and fourth chunk are ties; "observed": no
    tied step and no step in front of one is missing"""
    for c in E.TABLE:
        if not c.ties:
            continue
        i, C = E.inputs(c), E.host(c, True)["tries"][0][0]
        tau = np.diff(i["t"])
        tie = i["tie"]
        assert np.all(tau[tie[1:]] == 0.0) and np.all(tau[~tie[1:]] > 0.0)
        assert tie[1] and tie[c.T - 1] and tie[800:816].all() and tie[C] and tie[3 * C], (c.name, C)
        assert 0.19 <= tie.mean() <= 0.23
        if c.ties == 2:
            assert not i["mk"][tie].any() and not i["mk"][np.nonzero(tie)[0] - 1].any()


def test_the_declines_are_the_ones_the_table_names():
    """the plan's "forward warm-up longer than four chunks" ends the logpdf call of C-decline-plan-d2 behind two launches and switches the engine off for the
    bound model; the posterior call of the same series is served (its chunk grows with Wb)"""
    c = E.BY_NAME["C-decline-plan-d2"]
    lp, post = E.host(c, False), E.host(c, True)
    assert lp["why"] == "plan" and lp["state"] == -1 and lp["attempts"] == 2 and [t[1] for t in lp["tries"]] == [80, 160] and lp["tries"][0][0] == 72
    assert post["served"] == 1 and post["state"] == 1 and [t[:3] for t in post["tries"]] == [(72, 80, 72), (144, 160, 144), (144, 320, 144)]
    for nm, bits in (("E-negR-mid-d3", 12), ("E-inf-edge-d3", 8)):
        h = E.host(E.BY_NAME[nm], True)
        assert h["why"] == "values" and h["status"] == bits and h["state"] == (-1 if bits & 4 else 0)


if __name__ == "__main__":
    fmt = lambda tries: "; ".join("(%d, %d, %d) %d %.1e %.1e" % t for t in tries)      # noqa: E731
    for c in E.TABLE:
        if c.what == "draw":
            h = E.host(c)
            print("%-32s draw       %s" % (c.name, fmt(h.get("tries") or [(h["C"], h["W"], h["Wd"], h["status"], h["dist_f"], h["dist_d"])])))
        else:
            for post in (False, True):
                if (c.post if post else c.lp) is not None:
                    h = E.host(c, post)
                    print("%-32s %-10s %s %s" % (c.name, "posterior" if post else "logpdf", fmt(h["tries"]), h["why"]))
