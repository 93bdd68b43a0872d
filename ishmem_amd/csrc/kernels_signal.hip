// ishmem_amd — put with signal, signal set / add / fetch and the point-to-point waits behind the
// host blocking, _nbi and _on_stream forms (ishmem_put_signal, ishmemx_signal_set / add,
// ishmem_signal_fetch, ishmem_signal_wait_until, ishmem_<TN>_wait_until / _test; src/ishmem.h:640-705,
// :1320-1354, :1551-1552, src/signaling.cpp, src/synchronization.cpp).  Contract: DESIGN.md §3c.
//
// put_signal_kernel: ONE workgroup.  The payload is copied exactly as rma_copy_kernel<true> copies
// it (head < 16 B up to dest's 16-B boundary, 16-B items, tail < 16 B; local loads nontemporal, peer
// stores write-through sc0 sc1; every access on the vector path), the workgroup looping over the
// tiles.  Then EVERY wave waits for its own stores (s_waitcnt vmcnt(0): a write-through store is
// acknowledged once memory has it), the workgroup meets at its barrier, and one lane updates the
// signal word with one system-scope atomic.  The signal can therefore not pass a payload byte:
// cdna_hip_programming.md Guideline 16 recipe R1 at system scope (its Pitfall 14 — only the
// signalling lane's wave drained — is what the barrier after the drain of every wave rules out).
// Payloads above put_signal_fused_max_bytes are rma_copy_kernel's grid followed by signal_op_kernel
// on the same stream (runtime.cpp): the kernel boundary is the drain.
//
// signal_wait_kernel: one wave, one polling lane, relaxed system-scope loads, s_sleep back-off and a
// clock check every 16 polls (the shape of block_wait_ex); test and fetch are a budget of one poll.
#include "kernels_impl.h"

namespace ishmemi {
namespace {

constexpr int kSigBlock = kBlock, kSigUnroll = kUnroll;
constexpr uint64_t kSigTile = (uint64_t) kSigBlock * kSigUnroll;  // items per tile

__device__ __forceinline__ void signal_update(uint64_t *sig, uint64_t value, int sig_op)
{
    if (sig_op == kSignalAdd) (void) __hip_atomic_fetch_add(sig, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else __hip_atomic_store(sig, value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__global__ __launch_bounds__(kSigBlock) void put_signal_kernel(RmaArgs a, uint64_t *sig, uint64_t value, int sig_op)
{
    const uint32_t tid = threadIdx.x;
    const char *sb = a.src + a.head;
    char *db = a.dst + a.head;
    const uint64_t ntiles = (a.nitems + kSigTile - 1) / kSigTile;
    for (uint64_t t = 0; t < ntiles; ++t) {
        const uint64_t i0 = t * kSigTile;
        const uint32_t lim = (uint32_t) min((uint64_t) kSigTile, a.nitems - i0);
        // Descriptors based at the tile (offsets < 16 KiB, any payload size).
        const __amdgpu_buffer_rsrc_t lr = make_rsrc(uniform_ptr(sb + i0 * 16));
        const __amdgpu_buffer_rsrc_t dr = make_rsrc(uniform_ptr(db + i0 * 16));
        u32x4 x[kSigUnroll];
#pragma unroll
        for (int u = 0; u < kSigUnroll; ++u) {
            const uint32_t e = (uint32_t) u * kSigBlock + tid;
            if (e < lim) x[u] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(lr, e * 16u, 0, kNonTemporal));
        }
#pragma unroll
        for (int u = 0; u < kSigUnroll; ++u) {
            const uint32_t e = (uint32_t) u * kSigBlock + tid;
            if (e < lim) wt_store(dr, e * 16u, x[u]);
        }
    }
    // Head and tail bytes (< 16 each); descriptors based at the region.
    if (tid < 16) {
        for (int region = 0; region < 2; ++region) {
            const uint64_t cnt = region == 0 ? a.head : a.tail;
            const uint64_t rbase = region == 0 ? 0 : a.head + a.nitems * 16;
            if (tid >= cnt) continue;
            const uint8_t b = cload<uint8_t>(make_rsrc(a.src + rbase), tid);
            wt_store(make_rsrc(a.dst + rbase), tid, b);
        }
    }
    // Every storing wave drains, the workgroup meets, then ONE lane signals.
    drain_block();
    if (tid == 0) signal_update(sig, value, sig_op);
}

__global__ __launch_bounds__(64) void signal_op_kernel(uint64_t *sig, uint64_t value, int sig_op)
{
    if (threadIdx.x == 0) signal_update(sig, value, sig_op);
}

__device__ __forceinline__ uint64_t signal_poll(const WaitArgs &a)
{
    if (a.width == 8) return __hip_atomic_load((const uint64_t *) a.ivar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    const uint32_t v = __hip_atomic_load((const uint32_t *) a.ivar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return a.is_signed ? (uint64_t) (int64_t) (int32_t) v : (uint64_t) v;
}

__global__ __launch_bounds__(64) void signal_wait_kernel(WaitArgs a)
{
    if (threadIdx.x != 0) return;
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint64_t v = 0;
    int st = kWaitNoMatch;
    for (uint64_t it = 0;; ++it) {
        v = signal_poll(a);
        if (signal_compare(v, a.cmp, a.cmp_value, a.width, a.is_signed)) {
            st = kWaitMatched;
            break;
        }
        if (a.budget && it + 1 >= a.budget) break;
        if ((it & 15) == 15 && __builtin_amdgcn_s_memrealtime() - t0 > a.timeout_ticks) {
            st = kWaitTimedOut;
            if (a.err) __hip_atomic_fetch_or(a.err, kWaitErrBit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            break;
        }
        if (it < 32) __builtin_amdgcn_s_sleep(1);
        else __builtin_amdgcn_s_sleep(8);
    }
    if (a.value_out) __hip_atomic_store(a.value_out, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    if (a.status_out) {
        // The value first: a host that spins on the status word reads the value after it.
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(a.status_out, st, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

hipError_t launch_put_signal(const RmaArgs &a, uint64_t *sig, uint64_t value, int sig_op, hipStream_t s)
{
    hipLaunchKernelGGL(put_signal_kernel, dim3(1), dim3(kSigBlock), 0, s, a, sig, value, sig_op);
    return hipGetLastError();
}

hipError_t launch_signal_op(uint64_t *sig, uint64_t value, int sig_op, hipStream_t s)
{
    hipLaunchKernelGGL(signal_op_kernel, dim3(1), dim3(64), 0, s, sig, value, sig_op);
    return hipGetLastError();
}

hipError_t launch_signal_wait(const WaitArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(signal_wait_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ishmemi
