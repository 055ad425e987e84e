// Stationary-gain engine, STREAMING logpdf kernel (round 6): the log marginal likelihood of an LTI model with one noise
// variance, scalar observations and no missing data (lgssm.jl:147-165 on the reference's `Fill` layout) behind its head, as ONE kernel that
// reads y exactly once -- no halo, no pass before it, no wait for the host inside it.
//
// The steps behind the head are cut into R runs, one per wave; a wave streams its run tile by tile (64 lanes x N consecutive steps) through
// its own LDS slice and carries the filter state from tile to tile exactly.  Inside a tile a lane's zero-start end state is a table product
// (the recursion from zero), the lanes' start states come from one DPP scan, and the second sweep is the reference's recursion itself in the modal
// coordinates of the stationary closed loop, input-normalised (tgp_stream_form.hpp: every Modal handed to this unit is that form's, and the records,
// Wt and z0 are in its coordinates): r = u - fw . z, z' = M z + e u, u = y - hh.  A run does not know the state it starts from: it starts
// from zero and also accumulates V = sum_t w_t r_t over its first tile (w_t = fw' M^t: how a start state moves the innovations), so that
//     sum r^2 (start state s) = Q - 2 s . V + s' Wt s,   Wt = sum_t w_t' w_t  (data-free, from the host),
// to rounding once the tile is longer than the `halo` of the plan.  The waves of a workgroup apply that to each other after the one barrier
// at the kernel's end (s = the end state of the run before); the first run of every workgroup is closed by the HOST from the workgroups'
// (Q, V, E) triples in pinned memory -- and the head's end state z0 enters the same way, so the kernel never waits for the host.
#pragma once
#include <hip/hip_runtime.h>

#include "tgp_lml_record.hpp"
#include "tgp_steady_plan.hpp"

namespace tgp_lml {

constexpr int kNW = 8;            // waves per workgroup (one workgroup per CU: its LDS holds the eight tiles)
constexpr int kMaxWG = 512;       // workgroups of a launch at most (four waves per SIMD: two per CU; two: one per CU, 256)

struct Geometry {
    int n = 32;                    // steps per lane (16 or 32)
    int wps = 2;                   // waves per SIMD (2: one workgroup per CU; 4, n = 16 only: two)
    size_t lds = 0;                // dynamic LDS of the launch in bytes: with wps = 2, more than half a CU's, so that a CU takes ONE workgroup
    long long G = 0, R = 0, C = 1; // tiles of 64 n steps behind the head (the last one may be partial), runs (one wave each) that hold a tile, C = Chi
    long long W = 0, Chi = 1, Clo = 1;      // whole tiles; tiles per run of a workgroup's waves 0-3 / 4-7 (waves w and w + 4 share a SIMD)
    int nwg = 0;
    long long first_tile = 0;      // steps of a run's first tile (what Wt sums over)
};

// R runs over the G tiles behind the head; every run starts with a whole tile (>= halo) unless the series is shorter than that (then ONE run)
Geometry choose_geometry(const tgp_plan::Modal& md, long long T);

// pinned host memory the launch writes: part [nwg][record_lines(d)] LINES of 64 bytes (Q, V, E per workgroup, seven values and a check word to the line:
// tgp_lml_record.hpp) -- an area of this kernel's own, on a 64-byte boundary, cleared when it is allocated --, head_in [nhs], flags [0]: head_in is there
struct Buffers {
    double* part = nullptr;
    double* head_in = nullptr;
    long long* flags = nullptr;
};
constexpr size_t kStampOff = (size_t)kMaxWG * kLineWords * record_lines(tgp_plan::kMaxD);      // development stamps (TGP_LML_DBG) behind the largest record table
inline size_t part_doubles(int) { return kStampOff + 8 * (size_t)kMaxWG; }
// Have all records of call `seq` arrived?  *next: the first LINE not yet seen (0 at the first call; the scan resumes there).  With every record there
// the kernel has read all of y and written all it writes: the host may go on without synchronising the stream (which stays ordered).
bool records_there(const Geometry& g, int d, const double* part, long long seq, size_t* next);
// ... and the first n (value, check) PAIRS of a pair table of call `seq` (the streaming posterior kernel's: one pair per workgroup, tgp_post.hpp; check =
// the value's bits ^ record_key(seq))
bool records_there(size_t n, const double* part, long long seq, size_t* next);

// Wt = sum_{t < n} w_t' w_t (d x d, row-major), n = Geometry::first_tile -- data-free, O(d^2 log n) on the host
void quad_table(const tgp_plan::Modal& md, long long n, double* Wt);
// Enqueues the kernel on `stream` (no synchronisation).  0 or a hipError_t.
int enqueue(hipStream_t stream, const tgp_plan::Modal& md, const Geometry& g, long long T, const double* y, const Buffers& b, long long seq, const double* Wt,
            const char** kname);
// After flags[1] (or the stream) says the kernel is through: sum r^2 over the steps [nhs, T) given the head's end state z0 (the kernel's coordinates: tgp_stream_form::state_in)
double finish(const tgp_plan::Modal& md, const Geometry& g, const double* part, const double* z0, const double* Wt);

}  // namespace tgp_lml
