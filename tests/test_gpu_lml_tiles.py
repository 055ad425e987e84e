"""GPU tier: the streaming logpdf kernel (csrc/tgp_lml.hip) at the geometries whose tile length and wave slots are chosen separately
-- steps per lane and waves per SIMD, `tgp_lml::choose_geometry` -- against the oracle's sequential restatement (oracle/seq_kalman.c), 1e-10 relative
as in tests/test_gpu_stream.py.  Lengths sit around the edges of THAT geometry's tiles and runs; the kernel is named through the profile."""
import numpy as np
import pytest

from oracle import components as oc
from oracle import seq_kalman as sk

pytestmark = pytest.mark.gpu

KERNELS = {2: ("matern32",), 3: ("matern52",)}
# state dimension -> (steps per lane, waves per SIMD) of the default geometry: the headline's, and d = 2, which DESIGN 4.3's comparison moved
GEOMETRY = {2: (32, 2), 3: (32, 2)}
NHS = 64      # the head of these models at spacing 0.1, noise 0.1


def tile_of(d):
    return 64 * GEOMETRY[d][0]


def slots_of(d):      # wave slots of the chip: 256 CUs x 4 SIMDs x the waves per SIMD
    return 256 * 4 * GEOMETRY[d][1]


def lengths(d):
    tile = tile_of(d)
    return (NHS + tile - 1, NHS + tile, NHS + tile + 1, NHS + 2 * tile + 1,
            5000,                                # a partial last tile
            NHS + 17 * tile + 5,                 # C_hi != C_lo inside one workgroup
            300_001,
            slots_of(d) * tile + NHS + 17)       # the smallest length at which a run holds a second tile


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


_CASES = {}


def case(d, T, dt, s2, seed):
    """model, series and the oracle's logpdf of it: computed once per module"""
    key = (d, T, dt, s2, seed)
    if key not in _CASES:
        model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, dt, T), s2)
        rng = np.random.default_rng(seed)
        y = sk.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
        y.setflags(write=False)
        _CASES[key] = (model, y, sk.logpdf(model, y))
    return _CASES[key]


def device_model(tgp, model):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    dm.handle_options[tgp._lib.OPT_STREAM_MIN_T] = 0      # the streaming kernel at every length
    return dm


def logpdf_and_kernels(tgp, dm, y):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    lp = tgp.logpdf(dm, y)
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return lp, names


def kernel_name(d):
    return f"k_lml_stream<{GEOMETRY[d][0]}>"


@pytest.mark.parametrize("d,which", [(d, i) for d in sorted(GEOMETRY) for i in range(8)])
def test_lengths_around_the_tile_and_run_edges(tgp, d, which):
    T = lengths(d)[which]
    for dt, s2 in ((0.1, 0.1), (0.01, 1e-3)) if T < 100_000 else ((0.1, 0.1),):
        model, y, ref = case(d, T, dt, s2, 11 * d + which)
        lp, names = logpdf_and_kernels(tgp, device_model(tgp, model), y)
        print(f"d {d} T {T} dt {dt} s2 {s2}: relative difference {abs(lp - ref) / abs(ref):.3e} {sorted(names)}")
        assert abs(lp - ref) <= 1e-10 * abs(ref), (d, T, dt, lp, ref)
        if dt == 0.1:      # (the second noise setting has a longer head: below it the plan declines and the general engine serves)
            assert names == {kernel_name(d)}, (d, T, names)


@pytest.mark.parametrize("d", sorted(GEOMETRY))
def test_series_off_the_16_byte_boundary(tgp, d):
    import torch
    T = NHS + 17 * tile_of(d) + 5
    model, y, ref = case(d, T, 0.1, 0.1, 5)
    buf = torch.zeros(T + 1, dtype=torch.float64, device="cuda")
    buf[1:] = torch.from_numpy(y.copy()).cuda()
    assert buf[1:].data_ptr() % 16 == 8
    lp, names = logpdf_and_kernels(tgp, device_model(tgp, model), buf[1:])
    assert abs(lp - ref) <= 1e-10 * abs(ref), (d, lp, ref)
    assert names == {kernel_name(d)}, names


@pytest.mark.parametrize("d", sorted(GEOMETRY))
def test_records_of_an_earlier_call_do_not_pass_for_a_later_one(tgp, d):
    """three calls on ONE handle with different series: each must return its own value (the records carry the call's key)"""
    T = NHS + 17 * tile_of(d) + 5
    dm = None
    seen = []
    for seed in (5, 6, 7):
        model, y, ref = case(d, T, 0.1, 0.1, seed)
        dm = dm or device_model(tgp, model)
        lp, names = logpdf_and_kernels(tgp, dm, y)
        assert abs(lp - ref) <= 1e-10 * abs(ref), (d, seed, lp, ref)
        assert names == {kernel_name(d)}, names
        seen.append(ref)
    assert len({round(v, 3) for v in seen}) == 3      # (the three series really differ)
