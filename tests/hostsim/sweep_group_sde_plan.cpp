// Stand-alone host program around tgp_sweep_plan.hpp's plan_group for an SDE-described model (tests/test_sweep_group_sde_plan.py): no GPU, no HIP.
//   sweep_group_sde_plan MODEL_FILE T num_cu post fC fW fWb w_hint wb_hint
// MODEL_FILE: text, d then column-major: coef (lam d, N1 d*d, N2 d*d), a d, H d, hh, R, x0m d, Pinf d*d, A1 d*d, Q1 d*d, tau_typ.
// Prints "declined: <why>" or "ok d B owned C W Wb nchunks nwaves" followed by one line "span wave g t0 t1 runs owned" per group of every wave,
// then "x0m ..." and "x0P ..." (the state in front of update 0 as the kernel is given it, x0P by columns, d x d) and "N1 ..." (row-major, d x d).
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../temporalgps.jl_amd/csrc/tgp_sweep_plan.hpp"

int main(int argc, char** argv) {
    if (argc != 10) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    int d = 0;
    if (std::fscanf(f, "%d", &d) != 1 || d < 1 || d > 16) return 2;
    const size_t dd = (size_t)d * d;
    std::vector<double> v(5 * dd + 4 * (size_t)d + 3);
    for (double& x : v)
        if (std::fscanf(f, "%lf", &x) != 1) return 2;
    std::fclose(f);
    tgp_sweep::ModelHost m;
    m.d = d;
    m.sde = true;
    m.coef = v.data();
    m.a = m.coef + d + 2 * dd;
    m.H = m.a + d;
    m.hh = m.H[d];
    m.R = m.H[d + 1];
    m.x0m = m.H + d + 2;
    m.x0P = m.x0m + d;
    m.A = m.x0P + dd;
    m.Q = m.A + dd;
    m.tau_typ = m.Q[dd];
    const long long T = std::atoll(argv[2]);
    const int num_cu = std::atoi(argv[3]);
    const bool post = std::atoi(argv[4]) != 0;
    tgp_sweep::Forced fc;
    fc.C = std::atoi(argv[5]);
    fc.W = std::atoi(argv[6]);
    fc.Wb = std::atoi(argv[7]);
    tgp_sweep::GroupPlan p;
    std::string why;
    if (!tgp_sweep::plan_group(&p, fc, m, T, std::atoi(argv[8]), std::atoi(argv[9]), num_cu, post, &why)) {
        std::printf("declined: %s\n", why.c_str());
        return 0;
    }
    if (!p.sde) return 3;
    std::printf("ok %d %d %d %d %d %d %lld %lld\n", p.d, p.B, p.owned, p.C, p.W, p.Wb, (long long)p.nchunks, (long long)p.nwaves);
    for (long long w = 0; w < p.nwaves; ++w)
        for (int g = 0; g < tgp_sweep::kGroupsPerWave; ++g) {
            const tgp_sweep::GroupSpan s = tgp_sweep::group_span(w, g, p.owned, p.nchunks, p.C, p.T);
            std::printf("span %lld %d %lld %lld %d %d\n", w, g, s.t0, s.t1, (int)s.runs, (int)s.owned);
        }
    std::printf("x0m");
    for (int i = 0; i < d; ++i) std::printf(" %.17g", p.mc.x0m[i]);
    std::printf("\nx0P");
    for (int j = 0; j < d; ++j)
        for (int i = 0; i < d; ++i) std::printf(" %.17g", p.mc.x0P[i + 8 * j]);
    std::printf("\nN1");
    for (int i = 0; i < d; ++i)
        for (int k = 0; k < d; ++k) std::printf(" %.17g", p.sc.N1[8 * i + k]);
    std::printf("\n");
    return 0;
}
