"""GPU tier: logpdf + block gradients by the wide-state engine's adjoint pass (8 < d <= 63; csrc/tgp_wide.hip tgp_wide::adjoint, through tgp_logpdf_adjoint) placed
on the edges of its three device stages, against the oracle's exact sequential adjoint in long double (oracle/seq_adjoint.py; tests/test_oracle_adjoint.py holds it
to 1.1e-14 of 50-digit differences at d = 9 and 17 and shows that the double build agrees to 1e-14 at T = 2500 up to d = 63).

Bars.  logpdf: 1e-10 relative to seq_kalman.logpdf.  Every entry of every block: 1e-8 of the largest entry of the reference gradient (the project's gradient bar;
the CPU restatement of the algorithm stands within 1e-9 for every class here: tests/test_wide_adjoint_host.py).  Every entry of a block: within the class's and
block's own bar relative to the BLOCK's largest entry -- ten times the CPU restatement's figure, floored at 1e-10 (tests/_util.py WIDE_ADJOINT_MEASURED,
wide_adjoint_block_bar) -- so that a wrong entry in a block that weighs little in the whole gradient (x0m, x0P, a, h) is seen.
Classes: tests/_util.py WIDE_ADJOINT_KERNELS at spacing 0.2, noise 0.1, a = 0.01 linspace(-1, 1, d), h = 0.4; d = 9 at spacing 0.1 too.  (d = 14 at spacing 0.1
is left out on purpose: its restatement stands 3.9e-9 from the exact gradient, x0P 1.5e-7 of its own block -- the stationary head's cost, not a kernel's.)

Edges (every case asserts the whole profile label and, from tgp_wide_plan, the geometry it was built to hit):
  * k_wide_gram<NT>, NT = ceil((d + 2) / 16): the columns r_t (d) and 1 (d + 1) are the last two of the last tile at d = 14, 30, 46, 62 and split over two tiles at
    d = 15, 31, 47, 63; d = 15 / 16, 31 / 32, 47 / 48 are the form changes (k_wide_bwd4<1 .. 3, true>, k_wide_bwd<64, true>); NT = 5 at d = 63 alone.
  * the Gram spans: nw = min(2048, max(1, ceil(Tb / 256))) rounded up to a multiple of 4, span = ceil(Tb / nw) rounded up to a multiple of 4, Tb = T - n0: a partial
    last MFMA group (Tb mod 4 != 0), lam_T = 0 at t = T - 1, row n0 - 1 of m uploaded apart; above Tb = 2048 * 256 span > 256 and trailing waves are empty.
  * the ADJ backward kernels on the forward plan's chunks with a halo of their own: one chunk of exactly 64 steps, a last chunk of 1 and of 15 steps, forced counts
    of 1, 2, 3, 5, 7 chunks (TGP_WIDE_CHUNKS, child processes), 4065 and exactly 4096 chunks shorter than their warm-up.
  * one handle, three series, the last one a device tensor 8 bytes past a 16-byte boundary.

profiles/wide_adjoint_edges_parity.txt keeps, per class and block, the bar, the CPU restatement's figure and the largest deviation seen on an MI355X.

Mutation checks (one-line breaks of csrc/tgp_wide.hip in a scratch copy, run once each on an MI355X; only breaks that stay inside their buffers were run).  Run
against each: this file's 24 in-process tests of ordinary length -- every test but the forced chunk counts, whose child processes load the tree's own library, and
the two long series.
  * `a1 = a0 + span - 1` in k_wide_gram (every wave drops its last step): RUN.  All 24 in-process tests fail: A, a, Q, H, h, R stand 3e-3 ... 1e-1 of the largest
    entry from the oracle at every length from n0 + 64 on; x0m and x0P (the head's blocks, from lam at the head's end and the host pass) do not move.
  * `t + 2 < T` for `t + 1 < T` in k_wide_gram (lam_(T-1) taken as zero too): RUN.  All 24 fail: 1e-1 at n0 + 65, 2e-3 ... 2e-2 at T = 1500 ... 2500, 1.4e-4 for
    the third series on one handle -- one step's term.
  * `e->adj_halo / 4` in launch_backward (the backward warm-up a quarter as long): RUN.  22 fail and 2 pass: every default-plan case (4e-8 at d = 15, 2e-7 at
    d = 63), both Gram-span tests (a length of one chunk is untouched: n0 + 65 stands at 1.8e-14 at d = 12), all four last-chunk cases (9e-7 at d = 12), the three series
    (1.2e-8 ... 2.7e-7).  test_small_lengths_behind_the_head[28] and [63] pass, as they must: one chunk starts at T, where lam = 0 is exact and no halo is read.
    Deviations of 1e-8 ... 1e-6 of the largest entry: the 2e-6 bar of the directional checks in tests/test_gpu_wide_adjoint.py leaves room for them.
  * the upload of row n0 - 1 of m left out (a zero row uploaded in its place): RUN.  All 24 fail in A and H alone (the blocks that read m_(t-1) at t = n0: 5e-5 ...
    1e-1 of their own largest entry; 2.6e-5 of the whole gradient for the third series on one handle); a, Q, h, R, x0m, x0P do not move.
  * `t <= a1` for `t < a1` in k_wide_gram, `t <= g.s1` in the backward kernels' ownership: ARGUED FROM THE CODE, NOT RUN -- at the series' end they read r[T] and
    write lamT[T d + .], past the end of device buffers.  Elsewhere each counts (writes) one step twice at every wave (chunk) border: a relative change of the sums
    of order nw / Tb >= 1 / 260 against bars of 1e-8, as the first break above, which every case saw."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import seq_adjoint as sa
from oracle import seq_kalman as sk
from tests import _util as U

pytestmark = pytest.mark.gpu

BLOCKS = U.GRADIENT_BLOCKS
LP_BAR, GRAD_BAR = 1e-10, 1e-8
DT = 0.2
FORM_AND_GRAM_D = (9, 14, 15, 16, 17, 30, 31, 32, 33, 46, 47, 48, 49, 62, 63)
SPAN_TB = (64, 65, 66, 67, 80, 255, 256, 257, 1023, 1024, 1025, 1027)      # (80: the small lengths' third one)
GEOMETRY_D = (12, 28, 42, 54)      # NB = 1, 2, 3 and the LDS form
FORCED_T = 3000
# the default plan of every class at wide_adjoint_length(d), as tgp_wide_plan reports it: d -> (n0, halo, chunks, chunk_len)
DEFAULT_PLAN = {
    9: (27, 80, 38, 66), 14: (56, 216, 22, 112), 15: (50, 152, 32, 77), 16: (59, 200, 24, 102), 17: (62, 184, 26, 94), 30: (49, 144, 34, 73),
    31: (50, 152, 32, 77), 32: (61, 216, 22, 111), 33: (48, 160, 30, 82), 46: (59, 208, 13, 111), 47: (50, 152, 19, 77), 48: (61, 216, 13, 111),
    49: (52, 168, 17, 86), 62: (60, 176, 16, 90), 63: (48, 168, 17, 86),
}
_CASES = {}
WORST = {}      # (d, dt) -> {block or "lp" or "global": largest deviation seen}


def adjoint_label(d):
    return "k_wide_adjoint: " + U.wide_form_label(d) + " + k_wide_bwd + k_wide_gram"


def gram_geometry(Tb):
    """(waves, span) of the Gram reduction for Tb steps behind the head, as tgp_wide::adjoint computes them"""
    nw = min(2048, max(1, -(-Tb // 256)))
    nw = -(-nw // 4) * 4
    span = -(-Tb // nw)
    return nw, -(-span // 4) * 4


class Case:
    """a class's model, its draws and the oracle's logpdf and gradients, computed once per module and process"""

    def __init__(self, d, dt):
        self.d, self.dt, self._ref = d, dt, {}

    def model(self, T):
        return U.wide_adjoint_model(self.d, self.dt, T)

    def ref(self, T, seed=17, scale=1.0):
        """-> (y, logpdf, gradient) of the draw `seed` of length T (scaled: another series of the same model)"""
        key = (int(T), seed, scale)
        if key not in self._ref:
            m = self.model(T)
            y = scale * U.wide_adjoint_draw(m, seed)
            self._ref[key] = (y, sk.logpdf(m, y), sa.logpdf_adjoint(m, y)[1])
        return self._ref[key]


def case_of(d, dt=DT):
    if (d, dt) not in _CASES:
        _CASES[(d, dt)] = Case(d, dt)
    return _CASES[(d, dt)]


def compare(case, tag, lp, g, names, lp_ref, g_ref, failures):
    """one result against the oracle's: the bars of the module docstring; what misses goes to `failures`, the figures to WORST and to the output"""
    d, dt = case.d, case.dt
    dlp = abs(lp - lp_ref) / abs(lp_ref)
    glob, own = U.gradient_deviations(g, g_ref)
    print(f"d {d} dt {dt} {tag}: lp {dlp:.1e} global {max(glob.values()):.1e} | own " + " ".join(f"{k} {v:.1e}" for k, v in own.items()))
    w = WORST.setdefault((d, dt), {})
    for k, v in list(own.items()) + [("lp", dlp), ("global", max(glob.values()))]:
        w[k] = max(w.get(k, 0.0), v)
    if names != {adjoint_label(d)}:
        failures.append((d, tag, "label", sorted(names)))
    if not dlp <= LP_BAR:
        failures.append((d, tag, "lp", dlp))
    failures.extend((d, tag, "global " + k, v) for k, v in glob.items() if not v <= GRAD_BAR)
    failures.extend((d, tag, "own " + k, v, U.wide_adjoint_block_bar(d, dt, k)) for k, v in own.items() if not v <= U.wide_adjoint_block_bar(d, dt, k))


def check(tgp, case, T, failures, tag, seed=17, scale=1.0, y_dev=None, dm=None):
    """logpdf_adjoint of one series on a fresh handle (or on dm) against the oracle"""
    from temporalgps_jl_amd import lgssm as L
    y, lp_ref, g_ref = case.ref(T, seed, scale)
    dm = U.device_model(tgp, case.model(T)) if dm is None else dm
    (lp, g), names = U.kernels_of(tgp, dm, lambda: L.logpdf_adjoint(dm, y if y_dev is None else y_dev))
    compare(case, f"T {T} {tag}", lp, g, names, lp_ref, g_ref, failures)
    return g


def report(d, dt=DT):
    w = WORST.get((d, dt), {})
    print(f"PARITY d {d} dt {dt}: " + " ".join(f"{k} {w.get(k, 0.0):.1e}/{U.wide_adjoint_block_bar(d, dt, k):.1e}" for k in BLOCKS)
          + f" | global {w.get('global', 0.0):.1e}/{GRAD_BAR:.0e} lp {w.get('lp', 0.0):.1e}/{LP_BAR:.0e}")


@pytest.fixture(scope="module")
def tgp():
    import temporalgps_jl_amd as t
    t._lib.load()
    return t


# --------------------------------------------------------------------------- every form and Gram tile edge, the default plan
@pytest.mark.parametrize("d", FORM_AND_GRAM_D)
def test_every_form_and_gram_tile_edge_on_the_default_plan(tgp, d):
    T = U.wide_adjoint_length(d)
    case = case_of(d)
    pl = U.wide_plan(case.model(T), T)
    print(f"d {d}: T {T} plan {pl} Gram tiles {(d + 2 + 15) // 16} waves x span {gram_geometry(T - pl['n0'])}")
    assert pl["why"] == 0 and (pl["n0"], pl["halo"], pl["chunks"], pl["chunk_len"]) == DEFAULT_PLAN[d], (d, pl)
    assert pl["chunks"] >= 13 and ((T - pl["n0"]) % pl["chunk_len"] != 0) == (d != 62)      # (many chunks, the last one shorter; d = 62: 16 x 90 steps exactly)
    failures = []
    check(tgp, case, T, failures, "default plan")
    report(d)
    assert not failures, failures


# --------------------------------------------------------------------------- the Gram spans and the small lengths
def lengths_behind_the_head(tgp, d, Tbs):
    case = case_of(d)
    n0 = U.wide_plan(case.model(3000), 3000)["n0"]
    # one step short of the shortest series: declined, never a wrong value
    short = case.model(n0 + 63)
    assert U.wide_plan(short, n0 + 63)["why"] != 0
    from temporalgps_jl_amd import lgssm as L
    with pytest.raises(tgp._lib.Unsupported):
        L.logpdf_adjoint(U.device_model(tgp, short), case.ref(n0 + 64)[0][:n0 + 63])
    failures = []
    for Tb in Tbs:
        T = n0 + Tb
        pl = U.wide_plan(case.model(T), T)
        nw, span = gram_geometry(Tb)
        assert pl["why"] == 0 and pl["n0"] == n0, (Tb, pl)
        assert (pl["chunks"] - 1) * pl["chunk_len"] < Tb <= pl["chunks"] * pl["chunk_len"], (Tb, pl)
        if Tb < 128:
            assert (pl["chunks"], pl["chunk_len"]) == (1, Tb), (Tb, pl)          # one chunk of exactly Tb steps
        assert nw % 4 == 0 and span % 4 == 0 and nw * span >= Tb, (Tb, nw, span)
        check(tgp, case, T, failures, f"= n0 + {Tb}: {pl['chunks']} x {pl['chunk_len']}, {nw} waves x {span}")
    report(d)
    assert not failures, failures


@pytest.mark.parametrize("d", (12, 15))
def test_gram_spans_at_one_and_two_tiles(tgp, d):
    """d = 12: NT = 1; d = 15: NT = 2 with r_t in the first tile's last column and the constant in the second tile's first.  Tb = 64 ... 67: four waves of 16 or 20
    steps, Tb mod 4 = 0, 1, 2, 3 (a partial last MFMA group); 255 / 256 / 257: one block of four waves / the first length of two blocks; 1023 ... 1027: four and
    five blocks' worth (eight waves, the last ones short or empty).  One handle per length; n0 + 63 is declined."""
    assert [Tb % 4 for Tb in SPAN_TB[:4]] == [0, 1, 2, 3] and gram_geometry(256) == (4, 64) and gram_geometry(257) == (4, 68) and gram_geometry(1025) == (8, 132)
    assert (d + 2 + 15) // 16 == (1 if d == 12 else 2)
    lengths_behind_the_head(tgp, d, SPAN_TB)


@pytest.mark.parametrize("d", (28, 63))
def test_small_lengths_behind_the_head(tgp, d):
    """one chunk of exactly 64 steps, the first partial 16-block behind it (65), a full fifth 16-block (80): the gradient, not only the logpdf"""
    lengths_behind_the_head(tgp, d, (64, 65, 80))


# --------------------------------------------------------------------------- a last chunk of a few steps
def length_with_last_chunk_of(n0, halo, last):
    """the shortest length behind the head whose plan ends in a chunk of `last` steps (the search restates plan()'s rule; the test asserts what the plan reports)"""
    hm = max(64, halo // 2)
    for Tb in range(2 * hm + 1, 40 * hm * hm):
        c0 = max(1, min(4096, Tb // 64, Tb // hm))
        ln = -(-Tb // c0)
        c = -(-Tb // ln)
        if c >= 2 and Tb - (c - 1) * ln == last:
            return n0 + Tb
    raise AssertionError("no such length")


@pytest.mark.parametrize("d", (12, 42))
@pytest.mark.parametrize("last", (1, 15))
def test_a_last_chunk_of_a_few_steps(tgp, d, last):
    case = case_of(d)
    pl0 = U.wide_plan(case.model(3000), 3000)
    T = length_with_last_chunk_of(pl0["n0"], pl0["halo"], last)
    pl = U.wide_plan(case.model(T), T)
    got = (T - pl["n0"]) - (pl["chunks"] - 1) * pl["chunk_len"]
    print(f"d {d}: T {T} plan {pl} last chunk {got}")
    assert pl["why"] == 0 and got == last and pl["chunks"] >= 2 and T <= 6000, (pl, got, T)
    failures = []
    check(tgp, case, T, failures, f"last chunk of {last}")
    report(d)
    assert not failures, failures


# --------------------------------------------------------------------------- forced chunk counts (child processes)
def child_check(path, dims, chunks):
    """(runs in the child) the adjoint of every d in dims on the references the parent stored; the forced chunk count asserted from the plan"""
    import temporalgps_jl_amd as tgp
    from temporalgps_jl_amd import lgssm as L
    tgp._lib.load()
    failures = []
    for d in dims:
        r = dict(np.load(os.path.join(path, f"adj{d}.npz")))
        y, T = r["y"], len(r["y"])
        case = case_of(d)
        model = case.model(T)
        pl = U.wide_plan(model, T)
        assert pl["why"] == 0 and pl["chunks"] == chunks and pl["chunk_len"] == -(-(T - pl["n0"]) // chunks), (chunks, pl)
        dm = U.device_model(tgp, model)
        (lp, g), names = U.kernels_of(tgp, dm, lambda: L.logpdf_adjoint(dm, y))
        g_ref = {k: (float(r["g_" + k]) if k in ("h", "R") else r["g_" + k]) for k in BLOCKS}
        compare(case, f"T {T} forced {pl['chunks']} x {pl['chunk_len']}", lp, g, names, float(r["lp"]), g_ref, failures)
        report(d)
    print("FAILURES " + json.dumps([[str(x) for x in f] for f in failures]))
    print("checked")


@pytest.fixture(scope="module")
def stored_references(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("wide_adjoint_edges"))
    for d in GEOMETRY_D:
        y, lp, g = case_of(d).ref(FORCED_T)
        np.savez(os.path.join(path, f"adj{d}.npz"), y=y, lp=np.float64(lp), **{"g_" + k: np.asarray(g[k]) for k in BLOCKS})
    return path


CHILD = "import sys\nsys.path.insert(0, {root!r})\nfrom tests.test_gpu_wide_adjoint_edges import child_check\nchild_check({path!r}, {dims!r}, {chunks!r})\n"


@pytest.mark.parametrize("chunks", (1, 2, 3, 5, 7))
def test_forced_chunk_counts_under_the_adjoint_kernels(stored_references, chunks):
    """TGP_WIDE_CHUNKS (read once per process; it can only lower the count) at T = 3000, d = 12, 28, 42, 54: chunks many halos long under k_wide_bwd4<NB, true> /
    k_wide_bwd<64, true>, one to three invalid rows in the last DPP wave.  One child process per count, its own time limit, nothing retried."""
    r = subprocess.run([sys.executable, "-c", CHILD.format(root=U.ROOT, path=stored_references, dims=GEOMETRY_D, chunks=chunks)], capture_output=True, text=True,
                       timeout=300, env=dict(os.environ, TGP_WIDE_CHUNKS=str(chunks)), cwd=U.ROOT)
    print(r.stdout[-4000:])
    assert r.returncode == 0 and "checked" in r.stdout, (r.stdout + r.stderr)[-4000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("FAILURES ")][-1]
    assert json.loads(line[9:]) == [], line


# --------------------------------------------------------------------------- the second Gram regime and 4096 short chunks
@pytest.mark.parametrize("dt,Tb,halo,chunks,chunk_len,waves,span", [(0.1, 2048 * 256 + 1, 152, 4065, 129, 2048, 260), (0.2, 4096 * 70 - 5, 80, 4096, 70, 1120, 256)])
def test_the_second_gram_regime_and_thousands_of_chunks_shorter_than_their_warm_up(tgp, dt, Tb, halo, chunks, chunk_len, waves, span):
    """d = 9, y on the device, the oracle runs once per case (6 s and 0.8 GB; 3 s and 0.4 GB).
    Spacing 0.1 (halo 152), T = n0 + 2048 * 256 + 1: the plan asks for 4096 chunks, which makes them 129 steps long, and 524 289 steps are 4065 chunks of 129 -- the
    last wave has three invalid rows --, each shorter than its warm-up (forward and backward warm-ups cross a whole chunk and more); the Gram reduction's span is
    260 > 256 and its last 31 waves are empty (2048 x 260 - Tb = 8191 >= 260).
    Spacing 0.2 (halo 80), T = n0 + 4096 * 70 - 5: EXACTLY 4096 chunks of 70 steps, shorter than their warm-up, the last one five steps short.  (The same count at
    spacing 0.1, Tb = 4096 * 129 - 5, is left out: there the CPU restatement stands 1.09e-9 from the exact gradient, outside the 1e-9 a class needs for the 1e-8
    bar of this tier.)"""
    import torch
    case = case_of(9, dt)
    n0 = U.wide_plan(case.model(3000), 3000)["n0"]
    T = n0 + Tb
    pl = U.wide_plan(case.model(T), T)
    print(f"d 9 dt {dt}: T {T} plan {pl} waves x span {gram_geometry(Tb)}")
    assert pl["why"] == 0 and pl["n0"] == n0 and (pl["halo"], pl["chunks"], pl["chunk_len"]) == (halo, chunks, chunk_len) and pl["chunk_len"] < pl["halo"], pl
    assert gram_geometry(Tb) == (waves, span)
    if dt == 0.1:
        assert waves * span - Tb == 8191 and (waves * span - Tb) // span == 31
    failures = []
    y = case.ref(T)[0]
    check(tgp, case, T, failures, f"{chunks} x {chunk_len}, {waves} waves x {span}", y_dev=torch.from_numpy(y).cuda())
    report(9, dt)
    assert not failures, failures


# --------------------------------------------------------------------------- call sequences on one handle
def test_three_series_on_one_handle_each_get_their_own_gradient(tgp):
    """d = 28, T = 2500: the per-step scratch, the Gram partials and the pinned head state are the handle's; a second and a third series must not read the first's.
    The third is a device tensor 8 bytes past a 16-byte boundary."""
    import torch
    d, T = 28, 2500
    case = case_of(d)
    dm = U.device_model(tgp, case.model(T))
    failures, grads = [], []
    for i, (seed, scale) in enumerate(((17, 1.0), (18, 1.5), (19, 0.6))):
        y_dev = None
        if i == 2:
            buf = torch.zeros(T + 2, dtype=torch.float64, device="cuda")
            assert buf.data_ptr() % 16 == 0
            buf[1:T + 1] = torch.from_numpy(case.ref(T, seed, scale)[0]).cuda()
            y_dev = buf[1:T + 1]
            assert y_dev.data_ptr() % 16 == 8 and y_dev.is_contiguous()
        grads.append(check(tgp, case, T, failures, f"series {i} on one handle", seed=seed, scale=scale, y_dev=y_dev, dm=dm))
    report(d)
    assert not failures, failures
    assert np.abs(grads[0]["A"] - grads[1]["A"]).max() > 1e-3 * np.abs(grads[0]["A"]).max()      # (the series do differ)
