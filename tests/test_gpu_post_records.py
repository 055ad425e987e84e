"""GPU tier: the streaming posterior kernel's call ends on its workgroups' records in pinned memory, not on a stream synchronisation (csrc/tgp_post.hip,
tgp_modal.hip await_done): mean and var are stored write-through and acknowledged in front of the records, so a consumer on ANOTHER stream
(torch's) sees this call's outputs the moment the call returns.  The calls under test are made UNPROFILED -- a profiled call keeps the synchronising
end -- and the kernel's name is asserted in a separate, profiled call.  Oracle: oracle/seq_kalman.py; tolerances as everywhere: logpdf 1e-10
relative, mean and variance 1e-8 absolute."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import components as oc
from oracle import seq_kalman as sk

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = {1: ("matern12",), 2: ("matern32",), 3: ("matern52",)}
RN = 0.3
# no middle run (head + four tiles and a bit), a partial last tile behind five tiles, several runs, several runs with a partial last tile
LENGTHS = (5000, 5 * 1024 + 64 + 3, 100_000, 300_001)


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


def device_model(tgp, model):
    tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
    dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=model["T"])
    dm.handle_options[tgp._lib.OPT_STREAM_MIN_T] = 0      # (the streaming kernels at every length, as tests/test_gpu_stream.py)
    return dm


def kernels_of(tgp, dm, fn):
    hd = dm.handle()
    hd.set_option(tgp._lib.OPT_PROFILE, 1)
    hd.profile_reset()
    out = fn()
    names = set(hd.profile())
    hd.set_option(tgp._lib.OPT_PROFILE, 0)
    return out, names


@functools.lru_cache(maxsize=None)
def model_of(d, T):
    return oc.build_lgssm(KERNELS[d], ("regular", 0.0, 0.1, T), 0.1)


@functools.lru_cache(maxsize=None)
def case(d, T, seed):
    """(y, logpdf, mean, var) of the oracle with the shared new noise RN: computed once, shared between the tests, never written to"""
    model = model_of(d, T)
    rng = np.random.default_rng(seed)
    y = sk.rand(model, rng.standard_normal((T, d)), rng.standard_normal(T), rng.standard_normal(d))
    m, v = sk.posterior_marginals(model, y, np.array([RN]))
    for a in (y, m, v):
        a.setflags(write=False)
    return y, sk.logpdf(model, y), m, v


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def close(mean, var, m_ref, v_ref):
    return np.max(np.abs(mean.cpu().numpy() - m_ref)) <= 1e-8 and np.max(np.abs(var.cpu().numpy() - v_ref)) <= 1e-8


@pytest.mark.parametrize("d", (1, 2, 3))
def test_parity_on_the_records_end(tgp, d):
    import torch
    for T in LENGTHS:
        y, lp_ref, m_ref, v_ref = case(d, T, 3 * d + T % 11)
        dm = device_model(tgp, model_of(d, T))
        yd, Rd = dev(y), dev(np.array([RN]))
        out = (torch.zeros(T, dtype=torch.float64, device="cuda"), torch.zeros(T, dtype=torch.float64, device="cuda"))
        mean, var = tgp.posterior_marginals(dm, yd, Rd, out=out)
        assert close(mean, var, m_ref, v_ref), (d, T)
        out[0].zero_()
        out[1].zero_()
        torch.cuda.synchronize()
        lp, mean, var = tgp.logpdf_and_posterior_marginals(dm, yd, Rd, out=out)
        assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (d, T, lp, lp_ref)
        assert close(mean, var, m_ref, v_ref), (d, T)
        _, names = kernels_of(tgp, dm, lambda: tgp.posterior_marginals(dm, yd, Rd, out=out))
        assert names == {"k_post_stream"}, (d, T, names)


def test_same_bits_on_either_end(tgp):
    """one handle: an unprofiled call (records end) and a profiled one (synchronising end) -- the arithmetic is the same, so are the bits"""
    import torch
    d, T = 3, 300_001
    y, lp_ref, m_ref, v_ref = case(d, T, 1)
    dm = device_model(tgp, model_of(d, T))
    yd, Rd = dev(y), dev(np.array([RN]))
    lp1, mean1, var1 = tgp.logpdf_and_posterior_marginals(dm, yd, Rd)
    mean1, var1 = mean1.cpu().numpy(), var1.cpu().numpy()
    (lp2, mean2, var2), names = kernels_of(tgp, dm, lambda: tgp.logpdf_and_posterior_marginals(dm, yd, Rd))
    torch.cuda.synchronize()
    assert names == {"k_post_stream"}, names
    assert lp1 == lp2 and np.array_equal(mean1, mean2.cpu().numpy()) and np.array_equal(var1, var2.cpu().numpy())
    assert abs(lp1 - lp_ref) <= 1e-10 * abs(lp_ref) and np.max(np.abs(mean1 - m_ref)) <= 1e-8 and np.max(np.abs(var1 - v_ref)) <= 1e-8


def test_another_stream_sees_this_calls_outputs(tgp):
    """three calls with different series into the SAME output buffers; behind each, with no synchronisation in between, torch's current stream copies
    and reduces them: every copy is that call's result, not the one before -- then a second handle on the pooled stream"""
    import torch
    d, T = 3, 300_001
    dm = device_model(tgp, model_of(d, T))
    Rd = dev(np.array([RN]))
    out = (torch.zeros(T, dtype=torch.float64, device="cuda"), torch.zeros(T, dtype=torch.float64, device="cuda"))
    cases = [case(d, T, seed) for seed in (1, 2, 3)]
    yds = [dev(c[0]) for c in cases]
    torch.cuda.synchronize()
    for yd, (y, lp_ref, m_ref, v_ref) in zip(yds, cases):
        mean, var = tgp.posterior_marginals(dm, yd, Rd, out=out)
        m_copy, v_sum, v_copy = mean.clone(), var.sum(), var.clone()      # (torch's current stream, at once)
        assert np.max(np.abs(m_copy.cpu().numpy() - m_ref)) <= 1e-8
        assert np.max(np.abs(v_copy.cpu().numpy() - v_ref)) <= 1e-8
        assert abs(float(v_sum) - v_ref.sum()) <= 1e-8 * T      # (T terms, each within 1e-8)
    y, lp_ref, m_ref, v_ref = cases[0]
    dm2 = device_model(tgp, model_of(d, T))
    lp, mean, var = tgp.logpdf_and_posterior_marginals(dm2, yds[0], Rd, out=out)
    m_copy, v_copy = mean.clone(), var.clone()
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    assert close(m_copy, v_copy, m_ref, v_ref)


def test_fall_backs_keep_their_end(tgp):
    """a noise variance per step (plain stores), host arrays (copied back behind the kernel), outputs off the 16-byte boundary (k_steady_one): the
    synchronising end, the same results"""
    import torch
    d, T = 3, 300_001
    model = model_of(d, T)
    y, lp_ref, m_ref, v_ref = case(d, T, 1)
    dm = device_model(tgp, model)
    yd = dev(y)
    # per-step R_new
    Rn = np.random.default_rng(5).random(T) + 0.05
    ms_ref, vs_ref = sk.posterior_marginals(model, y, Rn)
    Rnd = dev(Rn)
    lp, mean, var = tgp.logpdf_and_posterior_marginals(dm, yd, Rnd)
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    assert close(mean, var, ms_ref, vs_ref)
    _, names = kernels_of(tgp, dm, lambda: tgp.posterior_marginals(dm, yd, Rnd))
    assert names == {"k_post_stream"}, names
    # host arrays in and out
    lp, mean, var = tgp.logpdf_and_posterior_marginals(dm, y, np.array([RN]))
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    assert np.max(np.abs(mean - m_ref)) <= 1e-8 and np.max(np.abs(var - v_ref)) <= 1e-8
    # outputs one element off the 16-byte boundary
    Rd = dev(np.array([RN]))
    buf_m, buf_v = torch.zeros(T + 1, dtype=torch.float64, device="cuda"), torch.zeros(T + 1, dtype=torch.float64, device="cuda")
    lp, mean, var = tgp.logpdf_and_posterior_marginals(dm, yd, Rd, out=(buf_m[1:], buf_v[1:]))
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref)
    assert close(mean, var, m_ref, v_ref)
    _, names = kernels_of(tgp, dm, lambda: tgp.posterior_marginals(dm, yd, Rd, out=(buf_m[1:], buf_v[1:])))
    assert all(n.startswith("k_steady_one") for n in names), names


def test_switch_gives_the_synchronising_end():
    """TGP_POST_RECORDS=0 (read once: a fresh child process): the same call, the same results"""
    code = """
import numpy as np, torch
import temporalgps_jl_amd as tgp
from oracle import components as oc
from oracle import seq_kalman as sk
T = 100_000
model = oc.build_lgssm(("matern52",), ("regular", 0.0, 0.1, T), 0.1)
rng = np.random.default_rng(4)
y = sk.rand(model, rng.standard_normal((T, 3)), rng.standard_normal(T), rng.standard_normal(3))
Rn = np.array([0.3])
m_ref, v_ref = sk.posterior_marginals(model, y, Rn)
lp_ref = sk.logpdf(model, y)
tr = tgp.GaussMarkovModel(tgp.Forward, model["A"], model["a"], model["Q"], tgp.Gaussian(model["x0m"], model["x0P"]))
dm = tgp.LGSSM(tr, tgp.ScalarOutputLGC(model["H"], np.atleast_1d(model["h"]), np.atleast_1d(model["R"])), T=T)
dm.handle_options[tgp._lib.OPT_STREAM_MIN_T] = 0
yd, Rd = torch.from_numpy(y).cuda(), torch.from_numpy(Rn).cuda()
for _ in range(2):
    lp, mean, var = tgp.logpdf_and_posterior_marginals(dm, yd, Rd)
    m, v = mean.clone().cpu().numpy(), var.clone().cpu().numpy()
    assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)
    assert np.max(np.abs(m - m_ref)) <= 1e-8 and np.max(np.abs(v - v_ref)) <= 1e-8
print("checked")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=dict(os.environ, TGP_POST_RECORDS="0"), cwd=ROOT)
    assert r.returncode == 0 and "checked" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_interleaved_logpdf_and_posterior_share_the_records(tgp):
    """k_lml_stream and k_post_stream write their records into the same pinned table: logpdf, posterior, logpdf on one handle with changing series"""
    d, T = 3, 300_001
    dm = device_model(tgp, model_of(d, T))
    Rd = dev(np.array([RN]))
    cases = [case(d, T, seed) for seed in (1, 2, 3)]
    yds = [dev(c[0]) for c in cases]
    for k in range(6):
        yd, (y, lp_ref, m_ref, v_ref) = yds[k % 3], cases[k % 3]
        if k % 2 == 0:
            lp = tgp.logpdf(dm, yd)
            assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (k, lp, lp_ref)
        elif k == 3:
            lp, mean, var = tgp.logpdf_and_posterior_marginals(dm, yd, Rd)
            assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (k, lp, lp_ref)
            assert close(mean, var, m_ref, v_ref), k
        else:
            mean, var = tgp.posterior_marginals(dm, yd, Rd)
            assert close(mean, var, m_ref, v_ref), k
    _, names = kernels_of(tgp, dm, lambda: tgp.logpdf(dm, yds[0]))
    assert all(n.startswith("k_lml_stream") for n in names), names


def test_fresh_handle_does_not_take_a_dropped_handles_records(tgp):
    """the record table is pinned memory from a recycling allocator and call numbers start at 1 with every handle: handle 1 makes ONE call and is
    dropped, handle 2's first call -- another series -- must wait for its own records and give its own results"""
    import gc
    d, T = 3, 300_001
    Rd = dev(np.array([RN]))
    cases = [case(d, T, seed) for seed in (1, 2)]
    yds = [dev(c[0]) for c in cases]
    for yd, (y, lp_ref, m_ref, v_ref) in zip(yds, cases):
        dm = device_model(tgp, model_of(d, T))
        lp, mean, var = tgp.logpdf_and_posterior_marginals(dm, yd, Rd)
        m_copy, v_copy = mean.clone(), var.clone()
        assert abs(lp - lp_ref) <= 1e-10 * abs(lp_ref), (lp, lp_ref)
        assert close(m_copy, v_copy, m_ref, v_ref)
        del dm, mean, var
        gc.collect()
