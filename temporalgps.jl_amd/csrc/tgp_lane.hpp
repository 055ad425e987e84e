// Lane primitives of the one-launch kernels (gfx950, wave64): DPP moves of a double, a wave talking to itself through LDS, the wave sum,
// and the bounded device-side wait for a flag in pinned host memory.  Every definition has internal linkage: each unit that includes this
// header gets its own copy, as when the text stood in the unit itself.
#pragma once
#include <hip/hip_runtime.h>

namespace {

typedef double v2d __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void lds_sync() {      // one wave talking to itself through LDS (DS operations of a wave execute in order)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The tables half of the host plan (per-step gains of the head, tail variances) may still be in the making when the kernel starts: the host
// writes the packed tables into pinned memory and then the flag 2 seq (+ 1 if that half declined: the call is then re-run elsewhere and
// whatever this kernel writes is discarded).  Workgroup 0 pulls them into device memory, all its waves at once (one PCIe round trip with
// every load in flight; a DMA copy of the same bytes reaches the device ~20 us after the API call)
// The wait is BOUNDED (round-4 advice): a host thread that dies between the launch and the flag, or a tool that makes the launch synchronous,
// would otherwise leave the queue spinning for ever.  After kWaitTicks of the 100 MHz clock (two seconds: the host half takes microseconds)
// the kernel goes on with whatever the table memory holds -- finite garbage at worst, every index comes from the arguments -- and poisons
// its share of the sum of squares (`poison`, when given), so that the call's result is NaN and is discarded.
constexpr long long kWaitTicks = 200000000ll;
__device__ __noinline__ void wait_tables(const long long* flagc, long long seq, double* poison = nullptr) {
    long long* flag = const_cast<long long*>(flagc);
    const long long t0 = (long long)wall_clock64();
    while (__hip_atomic_load(flag, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_SYSTEM) < 2 * seq) {
        __builtin_amdgcn_s_sleep(16);
        if ((long long)wall_clock64() - t0 > kWaitTicks) {
            if (poison != nullptr) *poison = __builtin_nan("");
            return;
        }
    }
}

__device__ __forceinline__ double readlane_d(double x, int l) {      // l wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), l), hi = __builtin_amdgcn_readlane(__double2hiint(x), l);
    return __hiloint2double(hi, lo);
}

// Data-parallel-primitive moves of a double (two 32-bit v_mov_dpp: no LDS round trip as ds_bpermute has).  Lanes without a source, and the
// rows the mask leaves out, read zero.  gfx9 controls: row_shl:n 0x100 + n (lane l reads l + n of its row of 16), row_shr:n 0x110 + n
// (reads l - n), wave_shl:1 0x130 / wave_shr:1 0x138 (the same across the whole wave), row_bcast:15 0x142 (lane 15 of a row to the next row),
// row_bcast:31 0x143 (lane 31 to rows 2, 3), row_newbcast:n 0x150 + n (lane n of a row to its own row)
template <int CTRL, int ROWMASK = 0xF>
__device__ __forceinline__ double dpp_mov(double x) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, ROWMASK, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, ROWMASK, 0xF, true);
    return __hiloint2double(hi, lo);
}
// the sum over the wave, in lane 63 (rows by row_shr adds, then row_bcast:15 / :31 across them)
__device__ __forceinline__ double wave_sum_to_lane63(double x) {
    x += dpp_mov<0x111>(x);
    x += dpp_mov<0x112>(x);
    x += dpp_mov<0x114>(x);
    x += dpp_mov<0x118>(x);
    x += dpp_mov<0x142, 0xA>(x);
    x += dpp_mov<0x143, 0xC>(x);
    return x;
}

}  // namespace
