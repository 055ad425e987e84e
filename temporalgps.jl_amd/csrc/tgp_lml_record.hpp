// The records of the streaming logpdf kernel (tgp_lml.hip): what a workgroup leaves in pinned host memory -- Q, V, E: 1 + 2 d values -- packed
// into LINES of 64 bytes, each written by ONE aligned 64-byte store of the workgroup and checked by the host a line at a time.  Plain C++: the kernel,
// the host and a host-only test (tests/test_lml_record_host.py) read the same text.
//
// A line holds seven values and one check word: the XOR of the seven values' bits with the call's key.  Value k of a record sits in line k / 7 at place
// k % 7; the places behind the last value hold zeros.  A line of THIS call is known when seen: the previous call's line carries another key even where
// its values are the same, a line with one stale value or a torn one (some sixteen-byte quarters old) does not add up unless the stale words equal the
// new ones -- then it holds the right values all the same --, and neither does a zeroed line or a line of four (value, check) pairs of the posterior
// kernel (three keys cancel to one, the check of the fourth pair cancels that: what is left is this call's key, never 0).
#pragma once

#if defined(__HIPCC__)
#define TGP_RECORD_HD __host__ __device__
#else
#define TGP_RECORD_HD
#endif

namespace tgp_lml {

constexpr int kLineValues = 7, kLineWords = 8;      // a line: seven values and the check word -- 64 bytes
static_assert(kLineWords == kLineValues + 1 && kLineWords * sizeof(unsigned long long) == 64, "a line is ONE 64-byte write: four sixteen-byte stores");

// lines of a record of 1 + 2 d values: d <= 3 one, d <= 6 two, d = 7, 8 three
TGP_RECORD_HD constexpr int record_lines(int d) { return (1 + 2 * d + kLineValues - 1) / kLineValues; }

// The call's key: a bijection of the call number, except that it is never 0 (the one call number that would give 0 gets the multiplier instead) -- a line
// or a pair of zeros must not pass for a record.  (The posterior kernel's pairs carry the same key: tgp_post.hip.)
TGP_RECORD_HD constexpr unsigned long long record_key(long long seq) {
    const unsigned long long k = (unsigned long long)seq * 0x9E3779B97F4A7C15ull + 0x632BE59BD9B4E019ull;
    return k != 0ull ? k : 0x9E3779B97F4A7C15ull;
}
static_assert(record_key(0) != 0ull && record_key(1) != 0ull && record_key(-1) != 0ull, "a zeroed record must not pass");

TGP_RECORD_HD inline unsigned long long record_bits(double v) {
    unsigned long long b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}

// the nv values of a record into its lines (8 words each), zeros behind the last value, every line's check word last
TGP_RECORD_HD inline void record_pack(int nv, const double* vals, unsigned long long key, unsigned long long* lines) {
    const int nl = (nv + kLineValues - 1) / kLineValues;
    for (int l = 0; l < nl; ++l) {
        unsigned long long x = key;
        for (int j = 0; j < kLineValues; ++j) {
            const int k = l * kLineValues + j;
            const unsigned long long b = k < nv ? record_bits(vals[k]) : 0ull;
            lines[l * kLineWords + j] = b;
            x ^= b;
        }
        lines[l * kLineWords + kLineValues] = x;
    }
}

// is this line one of the call with `key`?  (read word by word from memory another agent writes)
TGP_RECORD_HD inline bool record_line_ok(const volatile unsigned long long* line, unsigned long long key) {
    unsigned long long x = key;
    for (int j = 0; j < kLineValues; ++j) x ^= line[j];
    return x == line[kLineValues];
}

// value k of the record that starts at `rec` (a record's lines are consecutive)
TGP_RECORD_HD inline double record_value(const double* rec, int k) { return rec[(k / kLineValues) * kLineWords + k % kLineValues]; }

}  // namespace tgp_lml
