"""CPU tier: the ALGORITHM of the wide-state engine's adjoint pass (scripts/wide_adjoint_proto.py: chunked forward and backward recursions from zero
halos, the sums as one Gram matrix) against the sequential sums the host half reads (csrc/tgp_adjoint_host.hpp's record, as
tests/test_adjoint_host.py::device_like_record lays it out).  The HIP kernels: tests/test_gpu_wide_adjoint.py."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import components as oc
from oracle import lgssm_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {
    9: ("product", ("matern52",), ("stretched", 0.7, ("matern52",))),
    12: ("product", ("matern32",), ("approx_periodic", 3, 1.0)),
    28: ("product", ("approx_periodic", 7, 1.3), ("matern32",)),
}


@pytest.fixture(scope="module")
def proto():
    spec = importlib.util.spec_from_file_location("wide_adjoint_proto", os.path.join(ROOT, "scripts", "wide_adjoint_proto.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def sequential_sums(pl, y):
    """the record's sums over t >= n0 by the literal sequential recursions (the gain of step t: K_min(t, n0 - 1))"""
    T, d, n0 = len(y), pl["d"], pl["n0"]
    A, a, h, hh = pl["A"], pl["a"], pl["h"], pl["hh"]
    kA, S = A @ pl["K"], pl["S"]
    mu = A @ pl["x0m"] + a
    mus, rs = np.zeros((T, d)), np.zeros(T)
    for t in range(T):
        mus[t] = mu
        rs[t] = y[t] - hh - h @ mu
        mu = A @ mu + a + A @ pl["Ks"][min(t, n0 - 1)] * rs[t]
    psi = np.zeros(d)
    out = dict(SA=np.zeros((d, d)), Sa=np.zeros(d), Sk=np.zeros(d), Srm=np.zeros(d), Sr=0.0, SSQ=0.0)
    for t in range(T - 1, n0 - 1, -1):
        out["SA"] += np.outer(psi, mus[t])
        out["Sa"] += psi
        out["Sk"] += psi * rs[t]
        out["Srm"] += rs[t] * mus[t]
        out["Sr"] += rs[t]
        out["SSQ"] += rs[t] ** 2
        psi = A.T @ psi - h * (-rs[t] / S + kA @ psi)
    out["psi"], out["mu"] = psi, mus[n0]
    return out


@pytest.mark.parametrize("d", sorted(KERNELS))
@pytest.mark.parametrize("chunks", (1, 5))
def test_chunked_adjoint_sums_equal_the_sequential_ones(proto, d, chunks):
    T = 1600
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.2, T), 0.1)
    model["h"] = np.array([0.3])
    rng = np.random.default_rng(d)
    y = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    pl = proto.plan(model, T)
    assert pl is not None and pl["n0"] + 64 <= T and pl["halo_b"] is not None
    got, want = proto.sums(pl, y, chunks=chunks), sequential_sums(pl, y)
    for k, w in want.items():
        w = np.asarray(w)
        err = np.max(np.abs(np.asarray(got[k]) - w))
        assert err <= 1e-12 * max(1.0, np.abs(w).max()), (k, err, np.abs(w).max())


@pytest.mark.parametrize("d", sorted(KERNELS))
@pytest.mark.parametrize("geometry", ("two_chunks_per_halo", "four_chunks_per_halo", "last_chunk_of_a_few_steps"))
def test_chunks_shorter_than_the_backward_warm_up(proto, d, geometry):
    """chunks shorter than halo_b: a chunk's backward warm-up from zero crosses two (four) or more of the chunks ahead of it, as it does on the device when the plan
    makes thousands of chunks; and a count whose last chunk is 1 ... 15 steps (the series' end is then inside nearly every warm-up of the last halo_b steps)"""
    T = 1600
    model = oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.2, T), 0.1)
    model["h"] = np.array([0.3])
    model["a"] = 0.01 * np.linspace(-1.0, 1.0, d)[None]
    rng = np.random.default_rng(100 + d)
    y = ref.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    pl = proto.plan(model, T)
    assert pl is not None and pl["n0"] + 64 <= T and pl["halo_b"] is not None and pl["halo_b"] >= 16
    Tb, hb = T - pl["n0"], pl["halo_b"]
    if geometry == "last_chunk_of_a_few_steps":
        chunks = next(c for c in range(2, Tb) if 1 <= Tb - (-(-Tb // -(-Tb // c)) - 1) * -(-Tb // c) <= 15)
    else:
        chunks = -(-Tb // (hb // (2 if geometry == "two_chunks_per_halo" else 4)))
    ln = -(-Tb // chunks)
    n, last = -(-Tb // ln), Tb - (-(-Tb // ln) - 1) * ln
    print(f"d {d} {geometry}: halo_b {hb}, {n} chunks of {ln} steps, the last of {last}")
    if geometry == "last_chunk_of_a_few_steps":
        assert 1 <= last <= 15 and n >= 2
    else:
        assert ln * (2 if geometry == "two_chunks_per_halo" else 4) <= hb and n >= 8
    got, want = proto.sums(pl, y, chunks=chunks), sequential_sums(pl, y)
    for k, w in want.items():
        w = np.asarray(w)
        err = np.max(np.abs(np.asarray(got[k]) - w))
        assert err <= 1e-12 * max(1.0, np.abs(w).max()), (k, err, np.abs(w).max())
