// ishmem_amd — the atomic memory operations behind the host blocking and _nbi forms
// (ishmem_<TN>_atomic_<op>[_nbi], src/ishmem.h:331-640, src/amo.cpp, src/amo_impl.h).  Contract:
// DESIGN.md §3d.
//
// amo_kernel: one wave, one active lane, ONE relaxed system-scope operation on the word at `dest` (a
// PE's heap as mapped here): a load (fetch), a store (set) or a read-modify-write.  No AMO's result
// depends on signedness and float / double travel as bits, so the kernel knows only the width (4 or
// 8 bytes) and the operation; inc is add 1 (the runtime passes value = 1).  A fetching operation
// stores the old value to `fetch_out` (the runtime's pinned host word for the blocking call, the
// caller's `fetch` for _nbi) with a system-scope store of the same width; a non-fetching one uses the
// builtin's result nowhere, so the compiler emits the no-return instruction.  On gfx950 each builtin
// at system scope is one global_atomic_* instruction (sc0 sc1 with return, sc1 without), no
// compare-and-swap loop; every access is on the vector path.
#include "kernels_impl.h"

namespace ishmemi {
namespace {

template <typename U>
__device__ __forceinline__ void amo_one(const AmoArgs &a)
{
    U *p = (U *) a.dest;
    U *out = (U *) a.fetch_out;
    const U v = (U) a.value;
    constexpr int kOrder = __ATOMIC_RELAXED, kScope = __HIP_MEMORY_SCOPE_SYSTEM;
    U old = 0;
    switch (a.op) {
        case kAmoFetch: old = __hip_atomic_load(p, kOrder, kScope); break;
        case kAmoSet: __hip_atomic_store(p, v, kOrder, kScope); return;
        case kAmoSwap: old = __hip_atomic_exchange(p, v, kOrder, kScope); break;
        case kAmoCompareSwap: {
            U expected = (U) a.cond;
            (void) __hip_atomic_compare_exchange_strong(p, &expected, v, kOrder, kOrder, kScope);
            old = expected;  // the word's value before the operation, whether it matched or not
            break;
        }
        case kAmoFetchInc:
        case kAmoFetchAdd: old = __hip_atomic_fetch_add(p, v, kOrder, kScope); break;
        case kAmoFetchAnd: old = __hip_atomic_fetch_and(p, v, kOrder, kScope); break;
        case kAmoFetchOr: old = __hip_atomic_fetch_or(p, v, kOrder, kScope); break;
        case kAmoFetchXor: old = __hip_atomic_fetch_xor(p, v, kOrder, kScope); break;
        case kAmoInc:
        case kAmoAdd: (void) __hip_atomic_fetch_add(p, v, kOrder, kScope); return;
        case kAmoAnd: (void) __hip_atomic_fetch_and(p, v, kOrder, kScope); return;
        case kAmoOr: (void) __hip_atomic_fetch_or(p, v, kOrder, kScope); return;
        case kAmoXor: (void) __hip_atomic_fetch_xor(p, v, kOrder, kScope); return;
        default: return;
    }
    if (out) __hip_atomic_store(out, old, kOrder, kScope);
}

__global__ __launch_bounds__(64) void amo_kernel(AmoArgs a)
{
    if (threadIdx.x != 0) return;
    if (a.width == 8) amo_one<uint64_t>(a);
    else amo_one<uint32_t>(a);
}

}  // namespace

hipError_t launch_amo(const AmoArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(amo_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace ishmemi
