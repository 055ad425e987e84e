"""CPU tier: the input-normalised modal form of the streaming kernels (csrc/tgp_stream_form.hpp) as plain host C++.  A small main
builds modal forms by hand -- d = 1, 2, 3 and 6; closed loops with no conjugate pair, one pair, and pairs mixed with real modes; a non-zero emission
offset and a non-zero transition offset throughout -- and runs the plan's recursion and the normal form's side by side over 4 096 seeded steps:
    forward   the innovations, their sum of squares, the end state mapped back to the plan's coordinates;
    backward  the means, the left-edge state mapped back.
Every deviation is taken relative to the largest entry of what is compared and must stay within 1e-12: the two recursions are the same linear map in
two bases of one conditioning, so what separates them is rounding along a contracting recursion (a few hundred ulp at the spectral radii used here),
not a property of the model.  The guard: a model one of whose input coefficients is 1e-12 of the others reports that the form declines.
Given files, the same main reads a plan's modal form and a series from each and reports the case's largest deviation (tests/test_stream_envelope_host.py)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "temporalgps.jl_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
BOUND = 1e-12

MAIN = r"""
#include "tgp_stream_form.hpp"

#include <cmath>
#include <cstdio>
#include <vector>

using tgp_plan::Modal;
namespace sf = tgp_stream_form;

static unsigned long long rng_state = 0x243F6A8885A308D3ull;
static double uni() {      // (0, 1), splitmix64
    unsigned long long z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return ((double)(z >> 11) + 0.5) / 9007199254740992.0;
}
static double sym() { return 2.0 * uni() - 1.0; }
static double away() {      // a coefficient of either sign, 0.2 <= |c| <= 1.2
    const double m = 0.2 + uni();
    return uni() < 0.5 ? -m : m;
}

static int partner(int i, int np) { return i < 2 * np ? (i ^ 1) : i; }

// a modal form by hand: np conjugate pairs in front, real modes behind; spectral radii in [0.3, 0.9]
static Modal make(int d, int np, double hh, double offset) {
    Modal md{};
    md.d = d;
    md.npair = np;
    md.hh = hh;
    md.rS = 0.3;
    auto blocks = [&](double* re, double* im) {
        for (int i = 0; i < d; ++i) {
            if (i < 2 * np) {
                if (i & 1) continue;
                const double rho = 0.3 + 0.6 * uni(), th = 0.2 + 2.5 * uni();
                re[i] = re[i + 1] = rho * std::cos(th);
                im[i] = rho * std::sin(th);
                im[i + 1] = -im[i];
            } else {
                re[i] = (0.3 + 0.6 * uni()) * (uni() < 0.25 ? -1.0 : 1.0);
                im[i] = 0.0;
            }
        }
    };
    blocks(md.fd, md.fo);
    blocks(md.gd, md.go);
    for (int i = 0; i < d; ++i) {
        md.fb[i] = away();
        md.fa[i] = offset * sym();
        md.fw[i] = away();
        md.gc[i] = away();
        md.gw[i] = away();
    }
    return md;
}

static void step(int d, int np, const double* re, const double* im, const double* in, double u, const double* add, const double* z, double* nz) {
    for (int i = 0; i < d; ++i) {
        const int p = partner(i, np);
        nz[i] = re[i] * z[i] + (p != i ? im[i] * z[p] : 0.0) + in[i] * u + (add ? add[i] : 0.0);
    }
}

static double worst = 0.0;
static int fails = 0;
static void compare(const char* what, int d, int np, const std::vector<double>& a, const std::vector<double>& b) {
    double top = 0.0, dev = 0.0;
    for (size_t k = 0; k < a.size(); ++k) {
        top = std::fmax(top, std::fabs(a[k]));
        dev = std::fmax(dev, std::fabs(a[k] - b[k]));
    }
    const double rel = dev / top;
    worst = std::fmax(worst, rel);
    if (!(rel <= 1e-12)) {
        std::printf("FAIL d %d npair %d %s: %.3e\n", d, np, what, rel);
        ++fails;
    }
}

// the two recursions side by side on one modal form over 4096 steps.  series == nullptr: a seeded series around hh and a start state of the plan's;
// else the given series (4096 values) and a start state of unit size in the normal form's coordinates, mapped to the plan's by state_out
static void run_modal(const Modal& md, const double* series) {
    const int T = 4096, d = md.d, np = md.npair;
    const double hh = md.hh;
    sf::Form f;
    if (!sf::build(md, f)) {
        std::printf("FAIL d %d npair %d: the form declined\n", d, np);
        ++fails;
        return;
    }
    const Modal& nf = f.md;
    std::vector<double> y(T), r(T), rn(T), mean(T), meann(T);
    for (int t = 0; t < T; ++t) y[t] = series ? series[t] : hh + 3.0 * sym();
    double z[8], x[8], nz[8];
    if (series) {
        for (int i = 0; i < d; ++i) x[i] = sym();
        sf::state_out(f, x, z);
    } else {
        for (int i = 0; i < d; ++i) z[i] = 2.0 * sym();
    }
    sf::state_in(f, z, x);
    double q = 0.0, qn = 0.0;
    for (int t = 0; t < T; ++t) {
        const double u = y[t] - md.hh, un = y[t] - nf.hh;
        double a = u, b = un;
        for (int i = 0; i < d; ++i) {
            a -= md.fw[i] * z[i];
            b -= nf.fw[i] * x[i];
        }
        r[t] = a;
        rn[t] = b;
        q += a * a;
        qn += b * b;
        step(d, np, md.fd, md.fo, md.fb, u, md.fa, z, nz);
        for (int i = 0; i < d; ++i) z[i] = nz[i];
        step(d, np, nf.fd, nf.fo, nf.fb, un, nullptr, x, nz);      // (fb in {0, 1}: what the kernels compile in; no constant)
        for (int i = 0; i < d; ++i) x[i] = nz[i];
    }
    for (int i = 0; i < d; ++i)
        if (nf.fa[i] != 0.0 || (nf.fb[i] != 0.0 && nf.fb[i] != 1.0) || (nf.gc[i] != 0.0 && nf.gc[i] != 1.0)) {
            std::printf("FAIL d %d npair %d: not a normal form\n", d, np);
            ++fails;
        }
    compare("innovations", d, np, r, rn);
    compare("sum of squares", d, np, std::vector<double>{q}, std::vector<double>{qn});
    double back[8];
    sf::state_out(f, x, back);
    compare("end state", d, np, std::vector<double>(z, z + d), std::vector<double>(back, back + d));
    // backward, on the plan's innovations in both forms
    double ze[8] = {0}, xi[8] = {0};
    for (int t = T - 1; t >= 0; --t) {
        double m = y[t] - md.rS * r[t], mn = m;
        for (int i = 0; i < d; ++i) {
            m += md.gw[i] * ze[i];
            mn += nf.gw[i] * xi[i];
        }
        mean[t] = m;
        meann[t] = mn;
        step(d, np, md.gd, md.go, md.gc, r[t], nullptr, ze, nz);
        for (int i = 0; i < d; ++i) ze[i] = nz[i];
        step(d, np, nf.gd, nf.go, nf.gc, r[t], nullptr, xi, nz);
        for (int i = 0; i < d; ++i) xi[i] = nz[i];
    }
    compare("means", d, np, mean, meann);
    sf::zeta_out(f, xi, back);
    compare("left-edge backward state", d, np, std::vector<double>(ze, ze + d), std::vector<double>(back, back + d));
}

static void run(int d, int np, double hh, double offset) { run_modal(make(d, np, hh, offset), nullptr); }

// a plan's modal form and a series from a file: name, d, npair, hh, rS, then fd fo fb fa fw gd go gc gw (d values each), then 4096 observations.
// Prints the case's largest deviation; the caller holds it against the bound.
static int run_file(const char* path) {
    std::FILE* fp = std::fopen(path, "r");
    if (!fp) return 2;
    char name[64];
    Modal md{};
    bool ok = std::fscanf(fp, "%63s %d %d %lf %lf", name, &md.d, &md.npair, &md.hh, &md.rS) == 5 && md.d >= 1 && md.d <= 8 && md.npair >= 0 && 2 * md.npair <= md.d;
    double* arrs[9] = {md.fd, md.fo, md.fb, md.fa, md.fw, md.gd, md.go, md.gc, md.gw};
    for (int k = 0; ok && k < 9; ++k)
        for (int i = 0; ok && i < md.d; ++i) ok = std::fscanf(fp, "%lf", &arrs[k][i]) == 1;
    std::vector<double> y(4096);
    for (int t = 0; ok && t < 4096; ++t) ok = std::fscanf(fp, "%lf", &y[t]) == 1;
    std::fclose(fp);
    if (!ok) return 2;
    worst = 0.0;
    const int before = fails;
    run_modal(md, y.data());
    std::printf("case %s deviation %.3e%s\n", name, worst, fails == before ? "" : " FAIL");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {      // plans from files: one line per case, the exit status says only whether the files could be read
        for (int k = 1; k < argc; ++k)
            if (run_file(argv[k])) return 2;
        return 0;
    }
    const int grid[][2] = {{1, 0}, {2, 0}, {2, 1}, {3, 0}, {3, 1}, {6, 0}, {6, 1}, {6, 2}, {6, 3}};
    for (const auto& g : grid) {
        run(g[0], g[1], 0.7, 0.5);       // emission and transition offset
        run(g[0], g[1], -1.3, 0.0);      // emission offset alone: no shift to solve for
        run(g[0], g[1], 0.0, 0.25);      // transition offset alone
    }
    std::printf("largest deviation %.3e\n", worst);
    // the guard: one input coefficient at 1e-12 of the others
    {
        Modal md = make(3, 1, 0.7, 0.5);
        md.fb[2] *= 1e-12;
        sf::Form f;
        const bool ok = sf::build(md, f);
        std::printf("weak forward input: %s\n", ok || f.ok ? "served" : "declines");
        md = make(3, 1, 0.7, 0.5);
        md.gc[0] *= 1e-12;
        md.gc[1] *= 1e-12;
        const bool ok2 = sf::build(md, f);
        std::printf("weak backward input: %s\n", ok2 || f.ok ? "served" : "declines");
        md = make(3, 0, 0.7, 0.5);
        md.fb[1] = std::nan("");
        const bool ok3 = sf::build(md, f);
        std::printf("input not finite: %s\n", ok3 || f.ok ? "served" : "declines");
    }
    if (fails == 0) std::printf("stream form ok\n");
    return fails == 0 ? 0 : 1;
}
"""


def build_harness(tmp_path):
    """the main above, compiled for the host into tmp_path (tests/test_stream_envelope_host.py runs it on the plans of its table)"""
    src = tmp_path / "stream_form_main.cpp"
    exe = tmp_path / "stream_form_main"
    src.write_text(MAIN)
    # (no contraction: both recursions round every product and sum, as written)
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                            str(src), "-o", str(exe)], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return exe


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_normal_form_reproduces_the_plans_recursions_and_declines_a_weak_input(tmp_path):
    exe = build_harness(tmp_path)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "stream form ok" in run.stdout
    worst = float(re.search(r"largest deviation (\S+)", run.stdout).group(1))
    assert worst <= BOUND, worst
    for what in ("weak forward input", "weak backward input", "input not finite"):
        assert f"{what}: declines" in run.stdout
