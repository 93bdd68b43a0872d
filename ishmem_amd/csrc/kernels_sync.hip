// ishmem_amd — the vector waits and tests behind the host blocking and _on_stream forms of
// ishmem_<TN>_wait_until_all / _any / _some[_vector] and ishmem_<TN>_test_all / _any / _some[_vector]
// (src/ishmem.h:1343-1538, src/ishmemx.h:2043-2208, src/synchronization.cpp).  Contract: DESIGN.md §3f.
//
// sync_vector_kernel: ONE wave serves the six modes and both compare-value forms.  Lane l owns the
// elements base + u * 64 + l, u < kSyncUnroll, of the current chunk of kSyncChunk elements: a pass
// issues its kSyncUnroll relaxed system-scope loads (each of the variable's own width, never a wider
// one that spans neighbours) before it compares any of them, so several independent loads per lane
// are in flight.  Every decision that ends or continues a loop is made from a ballot or __all and is
// the same in all 64 lanes (cdna_hip_programming.md Guideline 16: one wave re-reads its words every
// pass, uniform exit).  Back-off and clock check have signal_wait_kernel's shape: s_sleep 1 for 32
// passes, then 8; s_memrealtime every 16 passes.  A test is a budget of one pass.
//   all:  the chunks are walked in order; a lane keeps, in a register, which of its elements of the
//         chunk were seen satisfied and does not load those again; the wave leaves the chunk when
//         every lane has none left.  Nothing is kept per element in memory.
//   any:  a pass sweeps every chunk; the winner, the first match in rotor order, comes from the
//         ballot masks alone (no second pass over memory).
//   some: the matching indices are compacted in ascending order from the ballot mask and the lane's
//         prefix count, with a running count across chunks, and written with ordinary vector stores.
// After a match ONE system-scope acquire and s_waitcnt vmcnt(0), then the results, another drain, and
// last the status word: a host that spins on the status word reads the results after it.
#include "kernels_impl.h"

namespace ishmemi {
namespace {

constexpr uint64_t kNone = ~0ull;

__device__ __forceinline__ uint64_t sync_poll(const void *ivars, uint64_t i, int width)
{
    if (width == 8) return __hip_atomic_load((const uint64_t *) ivars + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return (uint64_t) __hip_atomic_load((const uint32_t *) ivars + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The side arrays of one chunk: ok[u] = the lane's element u is inside the array and not excluded;
// cv[u] = its compare value.
__device__ __forceinline__ void sync_side(const SyncVecArgs &a, uint64_t base, uint32_t lane, bool (&ok)[kSyncUnroll],
                                          uint64_t (&cv)[kSyncUnroll])
{
#pragma unroll
    for (int u = 0; u < kSyncUnroll; ++u) {
        const uint64_t i = base + (uint64_t) u * 64 + lane;
        ok[u] = i < a.nelems;
        cv[u] = a.cmp_value;
        if (ok[u] && a.status) ok[u] = a.status[i] == 0;
        if (ok[u] && a.cmp_values)
            cv[u] = a.width == 8 ? ((const uint64_t *) a.cmp_values)[i] : (uint64_t) ((const uint32_t *) a.cmp_values)[i];
    }
}

__device__ __forceinline__ void sync_backoff(uint64_t it)
{
    if (it < 32) __builtin_amdgcn_s_sleep(1);
    else __builtin_amdgcn_s_sleep(8);
}

__device__ __forceinline__ bool sync_expired(const SyncVecArgs &a, uint64_t it, uint64_t t0)
{
    // wave-uniform: every lane reads the same scalar clock value
    return (it & 15) == 15 && __builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks;
}

// all modes.  Returns the status; base = the chunk the walk stopped in, left[u] = what is left of it.
__device__ __forceinline__ int sync_all(const SyncVecArgs &a, uint32_t lane, uint64_t t0, uint64_t &base,
                                        bool (&left)[kSyncUnroll])
{
    const bool test = sync_is_test(a.mode);
    uint64_t cv[kSyncUnroll];
    uint64_t it = 0;
    bool first = true;
    for (base = a.start; base < a.nelems; base += kSyncChunk) {
        sync_side(a, base, lane, left, cv);
        if (first) {
#pragma unroll
            for (int u = 0; u < kSyncUnroll; ++u) left[u] = left[u] && !((a.done_in[u] >> lane) & 1);
            first = false;
        }
        for (;; ++it) {
            uint64_t v[kSyncUnroll] = {};
#pragma unroll
            for (int u = 0; u < kSyncUnroll; ++u)
                if (left[u]) v[u] = sync_poll(a.ivars, base + (uint64_t) u * 64 + lane, a.width);
            bool pending = false;
#pragma unroll
            for (int u = 0; u < kSyncUnroll; ++u) {
                if (left[u] && signal_compare(v[u], a.cmp, cv[u], a.width, a.is_signed)) left[u] = false;
                pending |= left[u];
            }
            if (__all(!pending)) break;
            if (test) return kWaitNoMatch;
            if (sync_expired(a, it, t0)) return kWaitTimedOut;
            sync_backoff(it);
        }
    }
#pragma unroll
    for (int u = 0; u < kSyncUnroll; ++u) left[u] = false;
    return kWaitMatched;
}

// any and some modes.  result = the winner or kNone (any), the count (some).
__device__ __forceinline__ int sync_scan(const SyncVecArgs &a, uint32_t lane, uint64_t t0, uint64_t &result)
{
    const bool test = sync_is_test(a.mode), any = sync_is_any(a.mode);
    const bool single = a.nelems <= kSyncChunk;
    uint64_t start = 0;
    if (any && a.nelems) {
        const uint64_t r = a.rotor ? __hip_atomic_load(a.rotor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) : 0;
        start = (r % a.nelems + 1) % a.nelems;
    }
    bool ok[kSyncUnroll];
    uint64_t cv[kSyncUnroll];
    if (single) sync_side(a, 0, lane, ok, cv);  // one chunk: the side arrays are read once
    for (uint64_t it = 0;; ++it) {
        uint64_t count = 0, best_hi = kNone, best_lo = kNone;
        bool nonempty = false;
        for (uint64_t base = 0; base < a.nelems; base += kSyncChunk) {
            if (!single) sync_side(a, base, lane, ok, cv);
            uint64_t v[kSyncUnroll] = {};
#pragma unroll
            for (int u = 0; u < kSyncUnroll; ++u)
                if (ok[u]) v[u] = sync_poll(a.ivars, base + (uint64_t) u * 64 + lane, a.width);
#pragma unroll
            for (int u = 0; u < kSyncUnroll; ++u) {
                const uint64_t sb = base + (uint64_t) u * 64;
                const bool match = ok[u] && signal_compare(v[u], a.cmp, cv[u], a.width, a.is_signed);
                const uint64_t m = __ballot(match);
                if (it == 0) nonempty |= __ballot(ok[u]) != 0;
                if (m == 0) continue;
                if (any) {
                    if (best_lo == kNone) best_lo = sb + (uint64_t) __builtin_ctzll(m);
                    uint64_t mh = m;  // the matches at or after `start`
                    if (start > sb) mh = start - sb >= 64 ? 0 : m & (~0ull << (start - sb));
                    if (best_hi == kNone && mh) best_hi = sb + (uint64_t) __builtin_ctzll(mh);
                } else {
                    const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0));
                    if (match) a.indices[count + before] = (size_t) (sb + lane);
                    count += (uint64_t) __builtin_popcountll(m);
                }
            }
            if (any && best_hi != kNone) break;
        }
        if (any) result = best_hi != kNone ? best_hi : best_lo;
        else result = count;
        if (any ? result != kNone : count != 0) return kWaitMatched;
        if (it == 0 && !nonempty) return kWaitMatched;  // empty wait set: decided in the first pass
        if (test) return kWaitNoMatch;
        if (sync_expired(a, it, t0)) return kWaitTimedOut;
        sync_backoff(it);
    }
}

__global__ __launch_bounds__(64) void sync_vector_kernel(SyncVecArgs a)
{
    const uint32_t lane = threadIdx.x;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t result = 0, next = 0;
    bool left[kSyncUnroll] = {};
    int st;
    bool matched_something;
    if (sync_is_all(a.mode)) {
        st = sync_all(a, lane, t0, next, left);
        result = st == kWaitMatched ? 1 : 0;
        matched_something = st == kWaitMatched;
    } else {
        st = sync_scan(a, lane, t0, result);
        matched_something = st == kWaitMatched && (sync_is_any(a.mode) ? result != kNone : result != 0);
    }
    if (matched_something) {
        // ONE acquire after the match, and its invalidate has landed before any result is written.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    if (st == kWaitTimedOut && a.err && lane == 0)
        __hip_atomic_fetch_or(a.err, kWaitErrBit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    uint64_t done[kSyncUnroll];
#pragma unroll
    for (int u = 0; u < kSyncUnroll; ++u) done[u] = __ballot(!left[u]);
    if (lane == 0) {
        if (a.result_out) __hip_atomic_store(a.result_out, result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.next_out) __hip_atomic_store(a.next_out, next, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.done_out)
#pragma unroll
            for (int u = 0; u < kSyncUnroll; ++u)
                __hip_atomic_store(a.done_out + u, done[u], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (a.rotor && sync_is_any(a.mode) && matched_something)
            __hip_atomic_store(a.rotor, result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    if (a.status_out) {
        // The results (and the indices, whichever lanes stored them) first.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) __hip_atomic_store(a.status_out, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

hipError_t launch_sync_vector(const SyncVecArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(sync_vector_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ishmemi
