"""GPU tier: `bench.py --gpus 1` as every change is measured -- a plain run prints the headline line alone, and `--dump-outputs DIR`
writes what the last timed step returned (logpdf, posterior mean and variance of the bench's seeded series), held here against the
oracle's sequential restatement on the same series.  Tolerances as everywhere: logpdf 1e-10 relative, marginals 1e-8."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from oracle import components as oc
from oracle import seq_kalman as sk
from tests import _util as U

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_last_timed_step(tmp_path):
    import torch
    import temporalgps_jl_amd as tgp
    T = bench.DUMP_SAMPLE + 4099          # longer than the sample: the marginals are written at the fixed, seeded positions
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(U.ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--T", str(T),
           "--dump-outputs", str(tmp_path)]
    res = subprocess.run(cmd, env=env, cwd=U.ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout
    out = json.loads(lines[0])
    assert out["steps"] == 3 and out["unit"] == "Kalman steps/s" and out["higher_is_better"] is True and out["dtype"] == "f64"
    assert out["ms_per_step"] > 0 and abs(out["value"] - T / (out["ms_per_step"] * 1e-3)) <= 1e-9 * out["value"]
    assert "roofline" not in out and "cpu_baseline" not in out          # (--full)
    got = {n: np.load(tmp_path / f"{n}.npy") for n in ("logpdf", "mean", "var")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["logpdf"].shape == (1,) and got["mean"].shape == got["var"].shape == (bench.DUMP_SAMPLE,)

    # the bench's series, drawn as bench.py draws it (seeded device generator, the product's rand), through the oracle
    k, d, dt, s2 = bench.WORKLOADS["matern52_d3"]
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(123456)
    eps_t = torch.randn((T, d), dtype=torch.float64, device="cuda:0", generator=gen)
    eps_e = torch.randn((T,), dtype=torch.float64, device="cuda:0", generator=gen)
    y = tgp.rand((eps_t, eps_e, np.random.default_rng(0).standard_normal(d)), bench.build_model(tgp, "matern52_d3", T, "lti", 0))
    y = y.cpu().numpy()
    model = oc.build_lgssm(k, ("regular", 0.0, dt, T), s2)
    lp_ref = sk.logpdf(model, y)
    m_ref, v_ref = sk.posterior_marginals(model, y, np.array([1e-18]))
    assert abs(got["logpdf"][0] - lp_ref) <= 1e-10 * abs(lp_ref)
    assert float(np.max(np.abs(got["mean"] - bench.dump_sample(T, [(0, m_ref)])))) <= 1e-8
    assert float(np.max(np.abs(got["var"] - bench.dump_sample(T, [(0, v_ref)])))) <= 1e-8
