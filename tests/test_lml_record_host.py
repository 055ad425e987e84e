"""CPU tier: the record format of the streaming logpdf kernel (csrc/tgp_lml_record.hpp) -- lines of seven values and a check word -- as plain
host C++: the header is compiled with a small main of its own under AddressSanitizer and UndefinedBehaviorSanitizer and run.  What the host's wait
relies on: a complete line of this call passes; a zeroed line, the previous call's line with the same values, a line with one stale value, a torn line
whose check word is the old one and a line of four (value, check) pairs of the posterior kernel do not; the key is never 0; pack -> unpack round-trips
at every state dimension."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "temporalgps.jl_amd", "csrc")
CXX = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")

MAIN = r"""
#include "tgp_lml_record.hpp"

#include <cstdio>
#include <cstring>

using namespace tgp_lml;
typedef unsigned long long u64;

static int fails = 0;
#define CHECK(c)                                              \
    do {                                                      \
        if (!(c)) {                                           \
            std::printf("FAIL line %d: %s\n", __LINE__, #c);  \
            ++fails;                                          \
        }                                                     \
    } while (0)

static u64 bits(double v) {
    u64 b;
    std::memcpy(&b, &v, sizeof b);
    return b;
}

int main() {
    // lines of a record: d <= 3 one, d <= 6 two, d = 7 and 8 three
    const int want_lines[9] = {0, 1, 1, 1, 2, 2, 2, 3, 3};
    for (int d = 1; d <= 8; ++d) CHECK(record_lines(d) == want_lines[d]);
    static_assert(kLineWords * sizeof(u64) == 64, "a line is 64 bytes");

    // the key is never 0 -- not even at the one call number whose product cancels the offset (the multiplier is odd: its inverse by Newton's iteration)
    const u64 mul = 0x9E3779B97F4A7C15ull, off = 0x632BE59BD9B4E019ull;
    u64 inv = mul;
    for (int it = 0; it < 6; ++it) inv *= 2ull - mul * inv;
    CHECK(mul * inv == 1ull);
    const long long cancels = (long long)(inv * (0ull - off));
    CHECK((u64)cancels * mul + off == 0ull);
    CHECK(record_key(cancels) != 0ull);
    for (long long seq = -1000; seq <= 100000; ++seq) CHECK(record_key(seq) != 0ull);
    CHECK(record_key(4) != record_key(5));

    const long long seq = 5;
    const u64 key = record_key(seq), key_prev = record_key(seq - 1);
    const double vals[7] = {1234.5678, -0.25, 3.0e-300, -7.5e200, 0.0, 1.0, -1.0};
    u64 line[8], prev[8];
    record_pack(7, vals, key, line);
    record_pack(7, vals, key_prev, prev);

    // a complete line of this call passes, and holds the values
    CHECK(record_line_ok(line, key));
    for (int j = 0; j < 7; ++j) CHECK(line[j] == bits(vals[j]));

    // a zeroed line passes for no call
    const u64 zero[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    CHECK(!record_line_ok(zero, key));
    CHECK(!record_line_ok(zero, record_key(cancels)));
    for (long long s = 0; s <= 1000; ++s) CHECK(!record_line_ok(zero, record_key(s)));

    // the previous call's line with identical values does not pass for this call (it passes for its own)
    CHECK(record_line_ok(prev, key_prev));
    CHECK(!record_line_ok(prev, key));

    // one stale value -- any of the seven, or the check word -- and the line does not add up
    for (int j = 0; j < 8; ++j) {
        u64 stale[8];
        std::memcpy(stale, line, sizeof stale);
        stale[j] = j < 7 ? bits(vals[j]) + 1ull : prev[7];      // (the neighbouring double; the previous call's check word)
        CHECK(!record_line_ok(stale, key));
    }
    // a torn line (sixteen-byte quarters, some of the previous call with the same values): with the old check word it fails; with the new one every
    // word equals this call's, and it passes with the right values
    for (int mask = 1; mask < 15; ++mask) {
        u64 torn[8];
        for (int q = 0; q < 4; ++q) std::memcpy(torn + 2 * q, ((mask >> q) & 1 ? prev : line) + 2 * q, 16);
        const bool old_check = ((mask >> 3) & 1) != 0;
        CHECK(record_line_ok(torn, key) == !old_check);
    }

    // four (value, check) pairs of the posterior kernel in a line: of this very call, of the previous one
    for (int which = 0; which < 2; ++which) {
        const u64 pk = which == 0 ? key : key_prev;
        u64 pairs[8];
        for (int q = 0; q < 4; ++q) {
            pairs[2 * q] = bits(vals[q]);
            pairs[2 * q + 1] = bits(vals[q]) ^ pk;
        }
        CHECK(!record_line_ok(pairs, key));
    }

    // pack -> unpack at d = 1 ... 8: every line passes for its call only, the values come back bit for bit, the places behind the last value hold zeros
    for (int d = 1; d <= 8; ++d) {
        const int nv = 1 + 2 * d, nl = record_lines(d);
        double v[17];
        for (int k = 0; k < nv; ++k) v[k] = (k % 2 ? -1.0 : 1.0) * (0.1 + k) * (k % 3 == 0 ? 1e-12 : 1e7);
        v[nv - 1] = -0.0;
        u64 lines[3 * 8];
        for (int k = 0; k < 24; ++k) lines[k] = ~0ull;
        record_pack(nv, v, key, lines);
        double as_double[3 * 8];
        std::memcpy(as_double, lines, sizeof lines);
        for (int l = 0; l < nl; ++l) {
            CHECK(record_line_ok(lines + 8 * l, key));
            CHECK(!record_line_ok(lines + 8 * l, key_prev));
        }
        for (int k = 0; k < nv; ++k) CHECK(bits(record_value(as_double, k)) == bits(v[k]));
        for (int k = nv; k < 7 * nl; ++k) CHECK(lines[(k / 7) * 8 + k % 7] == 0ull);
        for (int k = 8 * nl; k < 24; ++k) CHECK(lines[k] == ~0ull);      // (nothing written behind the record's lines)
    }

    if (fails == 0) std::printf("record format ok\n");
    return fails == 0 ? 0 : 1;
}
"""


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_record_lines_pack_check_and_round_trip_under_sanitizers(tmp_path):
    src = tmp_path / "record_main.cpp"
    exe = tmp_path / "record_main"
    src.write_text(MAIN)
    build = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, str(src), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    print(run.stdout, run.stderr)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "record format ok" in run.stdout
