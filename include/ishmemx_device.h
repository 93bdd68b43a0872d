/* ishmem_amd — device-callable collectives, header-only HIP (included by ishmem.h / ishmemx.h
 * when the translation unit is compiled as HIP, so a kernel sees the reference's device API).
 *
 * Analogue of the reference's SYCL_EXTERNAL device API, called exactly as the reference calls it:
 *   ishmemx_<TYPENAME>_<op>_reduce_work_group([team,] dest, source, nreduce, grp)
 *       (src/ishmemx.h:1209-1803, src/collectives/reduce_impl.h:386-418, :505-518) — every thread
 *       of the group `grp` calls, on every PE of the team;
 *   ishmem_<TYPENAME>_<op>_reduce([team,] dest, source, nreduce) from ONE work-item (the
 *       reference's device-side blocking call, e.g. in a single_task: examples/6_team_split_strided.cpp:67);
 *   fcollect / collect / alltoall / sum_inscan / sum_exscan / broadcast in the same forms;
 *   ishmem_<TYPENAME>_put / _get / _p / _g, their _nbi, sized and mem forms from any work-item,
 *       ishmemx_*_{put,get}[_nbi]_work_group, ishmem_quiet / fence, ishmemx_quiet / fence_work_group;
 *   ishmem_<TYPENAME>_put_signal[_nbi], ishmemx_*_put_signal[_nbi]_work_group, ishmemx_signal_set / add,
 *       ishmem_signal_fetch / signal_wait_until, ishmem_<TYPENAME>_wait_until / _test and *_work_group;
 *   ishmem_<TYPENAME>_atomic_<op>[_nbi] and ishmem_atomic_<op>[_nbi]<T> from any work-item (ishmem_amo.h);
 *   ishmem_my_pe / n_pes / team_my_pe / team_n_pes / team_translate_pe / ptr / info_get_*,
 *   ishmem_barrier_all / sync_all / team_sync and their *_work_group forms, ishmemx_print.
 * `grp` is a HIP cooperative group — cooperative_groups::thread_block (the reference's
 * sycl::group) or a 64-lane cooperative_groups::thread_block_tile (its sycl::sub_group) — or one of
 * the tags ishmemx_dev::work_group / wavefront.
 *
 *   __global__ void k(int *dst, const int *src, size_t n) {
 *       auto grp = cooperative_groups::this_thread_block();
 *       ... produce src ...
 *       int rc = ishmemx_int_sum_reduce_work_group(dst, src, n, grp);
 *   }
 *
 * The library's device state reaches the kernel without an argument: every translation unit
 * that includes this header owns a device pointer to the library's context and registers it with
 * the library from a static initializer; ishmem_init fills every registered copy (a code object
 * loaded later is filled when it registers).  This is what SYCL device globals give the reference.
 *
 * Algorithm: the same direct reduce-scatter + all-gather as the host-launched kernel, executed by
 * the calling group (member c folds chunk c of every member's source in canonical team order
 * with system-coherent loads, stores it write-through, team barrier, then pulls the other chunks).
 * `source` must have been written by the calling group or by earlier kernels (the start barrier
 * releases this group's own writes).  Returns 0, or nonzero if the library is not initialised or
 * a peer did not arrive within the library's timeout.  dest/source must be symmetric-heap
 * addresses; source and dest identical or disjoint (reduce), disjoint (scan, collect, alltoall).
 */
#ifndef ISHMEM_AMD_ISHMEMX_DEVICE_H
#define ISHMEM_AMD_ISHMEMX_DEVICE_H

#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "ishmem_amo.h"
#include "ishmem_capi.h"
#include "ishmem_sync.h"
#include "ishmemx_fp16.h"

namespace ishmemx_dev {

// This translation unit's pointer to the library's device context (see the header comment).
static __device__ const ishmemi_c_device_ctx_t *g_ctx = nullptr;
[[maybe_unused]] static const int g_ctx_registered = ishmemi_c_register_device_ctx_slot((const void *) &g_ctx);

__device__ __forceinline__ const ishmemi_c_device_ctx_t *ctx() { return g_ctx; }

// The 16-bit floating-point types (ishmemx_fp16.h): round_to_nearest_even_T(f32(a) OP f32(b)) on
// the type's bits, the host kernels' fold — plain casts, no hand-written conversion.
template <typename T, int OP>
__device__ __forceinline__ T op1_fp16(T a, T b)
{
    static_assert(sizeof(T) == 2 && OP >= ISHMEMI_OP_MAX, "16-bit floating point: max, min, sum and prod only");
    constexpr bool half = ishmemi_cxx::fp16_kind<T>() == 1;
    const uint16_t ab = __builtin_bit_cast(uint16_t, a), bb = __builtin_bit_cast(uint16_t, b);
    float x, y, r;
    if constexpr (half) {
        x = (float) __builtin_bit_cast(_Float16, ab);
        y = (float) __builtin_bit_cast(_Float16, bb);
    } else {
        x = (float) __builtin_bit_cast(__bf16, ab);
        y = (float) __builtin_bit_cast(__bf16, bb);
    }
    if constexpr (OP == ISHMEMI_OP_MAX) r = fmaxf(x, y);
    else if constexpr (OP == ISHMEMI_OP_MIN) r = fminf(x, y);
    else if constexpr (OP == ISHMEMI_OP_SUM) r = x + y;
    else r = x * y;
    if constexpr (half) return __builtin_bit_cast(T, __builtin_bit_cast(uint16_t, (_Float16) r));
    else return __builtin_bit_cast(T, __builtin_bit_cast(uint16_t, (__bf16) r));
}

template <typename T, int OP>
__device__ __forceinline__ T op1(T a, T b)
{
    using W = std::conditional_t<(sizeof(T) == 8), uint64_t, uint32_t>;
    if constexpr (ishmemi_cxx::fp16_kind<T>() != 0) return op1_fp16<T, OP>(a, b);
    else if constexpr (OP == ISHMEMI_OP_AND) return (T) (a & b);
    else if constexpr (OP == ISHMEMI_OP_OR) return (T) (a | b);
    else if constexpr (OP == ISHMEMI_OP_XOR) return (T) (a ^ b);
    else if constexpr (OP == ISHMEMI_OP_MAX) {
        if constexpr (std::is_floating_point_v<T>) return fmax(a, b);
        else return (a < b) ? b : a;
    } else if constexpr (OP == ISHMEMI_OP_MIN) {
        if constexpr (std::is_floating_point_v<T>) return fmin(a, b);
        else return (b < a) ? b : a;
    } else if constexpr (OP == ISHMEMI_OP_SUM) {
        if constexpr (std::is_floating_point_v<T>) return a + b;
        else return (T) (std::make_unsigned_t<T>) ((W) (std::make_unsigned_t<T>) a + (W) (std::make_unsigned_t<T>) b);
    } else {
        if constexpr (std::is_floating_point_v<T>) return a * b;
        else return (T) (std::make_unsigned_t<T>) ((W) (std::make_unsigned_t<T>) a * (W) (std::make_unsigned_t<T>) b);
    }
}

// System-coherent element access (sc0 sc1): bypasses L1 / non-coherent L2 copies.
template <typename T>
__device__ __forceinline__ T sys_load(const T *p)
{
    using U = std::conditional_t<sizeof(T) == 8, uint64_t, std::conditional_t<sizeof(T) == 4, uint32_t,
              std::conditional_t<sizeof(T) == 2, uint16_t, uint8_t>>>;
    const U v = __hip_atomic_load((const U *) p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return __builtin_bit_cast(T, v);
}

template <typename T>
__device__ __forceinline__ void sys_store(T *p, T x)
{
    using U = std::conditional_t<sizeof(T) == 8, uint64_t, std::conditional_t<sizeof(T) == 4, uint32_t,
              std::conditional_t<sizeof(T) == 2, uint16_t, uint8_t>>>;
    __hip_atomic_store((U *) p, __builtin_bit_cast(U, x), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

__device__ __forceinline__ char *peer_addr(const ishmemi_c_device_ctx_t *c, const void *p, int pe)
{
    return c->peer_heap[pe] + ((const char *) p - c->heap_base);
}

// 16 bytes of T, the unit of the vectorised fold.
template <typename T>
struct alignas(16) Vec16 {
    T e[16 / sizeof(T)];
};
constexpr int kUnroll = 4;  // 16-B items in flight per thread and member
// The group's reduce-scatter loads this many members' items before folding them (a run-time loop
// over members would wait for each member's loads before issuing the next member's: 4 x 16 B per
// thread in flight), and the all-gather pulls this many 16-B items per thread per step.
#ifndef ISHMEMX_DEV_MEMBER_BATCH
#define ISHMEMX_DEV_MEMBER_BATCH 4
#endif
#ifndef ISHMEMX_DEV_AG_UNROLL
#define ISHMEMX_DEV_AG_UNROLL 8
#endif
constexpr int kMemberBatch = ISHMEMX_DEV_MEMBER_BATCH;
constexpr int kAgUnroll = ISHMEMX_DEV_AG_UNROLL;

template <typename T, int OP>
__device__ __forceinline__ Vec16<T> op16(const Vec16<T> &a, const Vec16<T> &b)
{
    Vec16<T> r;
#pragma unroll
    for (int i = 0; i < (int) (16 / sizeof(T)); ++i) r.e[i] = op1<T, OP>(a.e[i], b.e[i]);
    return r;
}

// A pointer every calling thread holds with the same value, moved to scalar registers (buffer
// descriptors need a uniform base; the group's threads all compute the same address).
__device__ __forceinline__ const char *group_uniform(const char *p)
{
    const uint64_t v = (uint64_t) p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t) v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t) (v >> 32));
    return (const char *) (((uint64_t) hi << 32) | lo);
}

// System-coherent (sc0 sc1) 16-B load / write-through store through a buffer descriptor based at
// `base`; off < 2 GiB.
template <typename T>
__device__ __forceinline__ Vec16<T> sys_load16(const char *base, uint32_t off)
{
    const __amdgpu_buffer_rsrc_t r =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), (short) 0, 0x7FFFFFFF, 0x00020000);
    return __builtin_bit_cast(Vec16<T>, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 17));
}

template <typename T>
__device__ __forceinline__ void sys_store16(char *base, uint32_t off, const Vec16<T> &v)
{
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(base, (short) 0, 0x7FFFFFFF, 0x00020000);
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), r, off, 0, 17);
}

// Execution groups that can call a device collective (the reference's `const Group &grp`:
// sycl::group<1..3> and sycl::sub_group, plus the single work-item of a device-side blocking
// call).  Every member of the group calls with identical arguments.
struct work_group_t {  // every thread of the work-group
    __device__ static int rank() { return threadIdx.x + blockDim.x * (threadIdx.y + blockDim.y * threadIdx.z); }
    __device__ static int size() { return blockDim.x * blockDim.y * blockDim.z; }
    __device__ static void sync() { __syncthreads(); }
    __device__ static uint32_t bcast(uint32_t v)
    {
        __shared__ uint32_t s_v;
        __syncthreads();
        if (rank() == 0) s_v = v;
        __syncthreads();
        return s_v;
    }
};
struct wavefront_t {  // one full 64-lane wavefront (sub_group analogue)
    __device__ static int rank() { return (int) __lane_id(); }
    __device__ static int size() { return warpSize; }
    __device__ static void sync() { __builtin_amdgcn_wave_barrier(); }
    __device__ static uint32_t bcast(uint32_t v) { return (uint32_t) __shfl((int) v, 0); }
};
struct thread_t {  // one work-item (device-side ishmem_<TN>_<op>_reduce)
    __device__ static int rank() { return 0; }
    __device__ static int size() { return 1; }
    __device__ static void sync() {}
    __device__ static uint32_t bcast(uint32_t v) { return v; }
};
inline constexpr work_group_t work_group{};
inline constexpr wavefront_t wavefront{};
inline constexpr thread_t thread{};

// Group argument -> execution tag: the library's tags, and HIP cooperative groups in the roles of
// the reference's sycl::group (thread_block) and sycl::sub_group (a 64-lane tile).
template <typename G>
struct exec_of {
    static_assert(std::is_same_v<G, work_group_t> || std::is_same_v<G, wavefront_t> || std::is_same_v<G, thread_t>,
                  "group: cooperative_groups::thread_block, thread_block_tile<64>, or an ishmemx_dev tag");
    using type = G;
};
template <>
struct exec_of<cooperative_groups::thread_block> {
    using type = work_group_t;
};
template <unsigned N, typename P>
struct exec_of<cooperative_groups::thread_block_tile<N, P>> {
    static_assert(N == 64, "a sub-group collective needs the whole 64-lane wavefront (thread_block_tile<64>)");
    using type = wavefront_t;
};
template <typename G>
using exec_t = typename exec_of<std::remove_cv_t<std::remove_reference_t<G>>>::type;

// Team barrier among the calling groups (one per member): the group's leader stores the epoch
// into its slot of every peer's row and polls its own row; bounded by the library timeout.
template <typename G>
__device__ inline bool group_barrier(const ishmemi_c_device_ctx_t *c, int team, int phase,
                                     uint32_t epoch, bool release)
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G::sync();
    uint32_t ok = 1;
    if (G::rank() == 0) {
        const int size = c->team_size[team], me = c->team_my_idx[team];
        const size_t row = ((size_t) team * ISHMEMI_C_DEV_PHASES + phase) * ISHMEMI_C_MAX_PES;
        if (release) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        for (int j = 0; j < size; ++j) {
            if (j == me) continue;
            const int gpe = c->team_start[team] + j * c->team_stride[team];
            __hip_atomic_store(c->peer_dflags[gpe] + row + me, epoch, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
        const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
        for (int j = 0; j < size && ok; ++j) {
            if (j == me) continue;
            while ((int32_t) (__hip_atomic_load(c->my_dflags + row + j, __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_SYSTEM) - epoch) < 0) {
                if (__builtin_amdgcn_s_memrealtime() - t0 > c->timeout_ticks) {
                    ok = 0;
                    __hip_atomic_fetch_or(c->err, 1u << phase, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
        }
        // One system-scope acquire by the leader drops this CU's stale L1 lines (and the L2's
        // non-coherent ones) for the whole group: bytes a peer PUT before the barrier are then read
        // by plain loads.  The leader waits for the invalidate before the group's barrier inside
        // bcast (a workgroup barrier waits for no memory counter), so every wave of the group, not
        // only the leader's, loads behind it.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    return G::bcast(ok) != 0;
}

template <typename G, typename T, int OP>
__device__ int reduce_group(const ishmemi_c_device_ctx_t *c, int team, T *dest, const T *source,
                            size_t nreduce)
{
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS) return 1;  // not initialised / bad handle
    const int tid = G::rank(), nthr = G::size();
    const int size = c->team_size[team], me = c->team_my_idx[team];
    if (size <= 0 || me < 0) return 1;
    uint32_t epoch = 0;
    if (tid == 0)
        epoch = __hip_atomic_fetch_add(c->epochs + team, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    epoch = G::bcast(epoch);
    if (size == 1) {  // one PE: dest = source (reduce_impl.h:288-289)
        if (dest != source)
            for (size_t i = tid; i < nreduce; i += nthr) dest[i] = source[i];
        G::sync();
        return 0;
    }
    // Start: every member's source is complete (this group's own writes released).
    if (!group_barrier<G>(c, team, 0, epoch, true)) return 1;
    const size_t per = ((nreduce + size - 1) / size + 63) & ~(size_t) 63;
    const size_t cs = (size_t) me * per < nreduce ? (size_t) me * per : nreduce;
    const size_t ce = cs + per < nreduce ? cs + per : nreduce;
    const int start = c->team_start[team], stride = c->team_stride[team];
    // 16-B items when both arrays are 16-B aligned (chunk edges are multiples of 64 elements, and
    // every heap is mapped at the same offsets, so peers' addresses share the residue); the few
    // elements of the last chunk past its last whole item, and misaligned arrays, go element-wise.
    constexpr size_t E = 16 / sizeof(T);
    const bool vec = ((((uintptr_t) dest) | ((uintptr_t) source)) & 15) == 0;
    const size_t nv = vec ? (ce - cs) / E : 0;
    for (size_t v0 = 0; v0 < nv; v0 += (size_t) nthr * kUnroll) {
        Vec16<T> acc[kUnroll];
        for (int j0 = 0; j0 < size; j0 += kMemberBatch) {
            Vec16<T> x[kMemberBatch][kUnroll];
#pragma unroll
            for (int b = 0; b < kMemberBatch; ++b) {
                const int j = j0 + b;
                if (j >= size) break;
                const int gpe = start + j * stride;
                const char *base = (j == me) ? (const char *) (source + cs) : peer_addr(c, source + cs, gpe);
                const char *step = group_uniform(base + v0 * 16);
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const size_t k = (size_t) u * nthr + tid;
                    if (v0 + k < nv) x[b][u] = sys_load16<T>(step, (uint32_t) (k * 16));
                }
            }
#pragma unroll
            for (int b = 0; b < kMemberBatch; ++b) {
                if (j0 + b >= size) break;
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) acc[u] = (j0 + b == 0) ? x[b][u] : op16<T, OP>(acc[u], x[b][u]);
            }
        }
        char *dstep = (char *) group_uniform((const char *) (dest + cs) + v0 * 16);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const size_t k = (size_t) u * nthr + tid;
            if (v0 + k < nv) sys_store16<T>(dstep, (uint32_t) (k * 16), acc[u]);  // write-through
        }
    }
    for (size_t i = cs + nv * E + tid; i < ce; i += nthr) {
        T acc = T();
        for (int j = 0; j < size; ++j) {
            const int gpe = start + j * stride;
            const T x = (j == me) ? source[i] : sys_load((const T *) peer_addr(c, source + i, gpe));
            acc = (j == 0) ? x : op1<T, OP>(acc, x);
        }
        sys_store(dest + i, acc);  // write-through: peers pull it after the next barrier
    }
    if (!group_barrier<G>(c, team, 1, epoch, true)) return 1;
    for (int k = 1; k < size; ++k) {
        const int j = (me + k) % size;
        const int gpe = start + j * stride;
        const size_t js = (size_t) j * per < nreduce ? (size_t) j * per : nreduce;
        const size_t je = js + per < nreduce ? js + per : nreduce;
        const size_t jv = vec ? (je - js) / E : 0;
        const char *pbase = peer_addr(c, dest + js, gpe);
        for (size_t v0 = 0; v0 < jv; v0 += (size_t) nthr * kAgUnroll) {
            const char *step = group_uniform(pbase + v0 * 16);
            Vec16<T> x[kAgUnroll];
#pragma unroll
            for (int u = 0; u < kAgUnroll; ++u) {
                const size_t q = (size_t) u * nthr + tid;
                if (v0 + q < jv) x[u] = sys_load16<T>(step, (uint32_t) (q * 16));
            }
            Vec16<T> *dp = (Vec16<T> *) (dest + js) + v0;
#pragma unroll
            for (int u = 0; u < kAgUnroll; ++u) {
                const size_t q = (size_t) u * nthr + tid;
                if (v0 + q < jv) dp[q] = x[u];
            }
        }
        for (size_t i = js + jv * E + tid; i < je; i += nthr)
            dest[i] = sys_load((const T *) peer_addr(c, dest + i, gpe));
    }
    // End: no member returns while a peer may still read its dest.
    return group_barrier<G>(c, team, 2, epoch, false) ? 0 : 1;
}

template <typename T, int OP>
__device__ int reduce_work_group(const ishmemi_c_device_ctx_t *c, int team, T *dest, const T *source,
                                 size_t nreduce)
{
    return reduce_group<work_group_t, T, OP>(c, team, dest, source, nreduce);
}

// Reduce-scatter from inside a kernel (extension): source holds `size` blocks of
// nreduce elements in the symmetric heap; this member folds block `me` of every member's source, in
// team order, into dest (nreduce elements, written by this group only: any memory the kernel can
// write).  reduce_group's start barrier (every source final), the fold — 16-B sys_load16 items,
// member-batched as in reduce_group, when this member's block and dest are both 16-B aligned,
// element-wise otherwise — and reduce_group's end barrier (no member returns while a peer may still
// read its source); no middle barrier and no all-gather.  The epoch comes from c->epochs like the
// siblings', so device reduces and reduce-scatters of one team may alternate.  dest overlapping
// source is undefined.
template <typename G, typename T, int OP>
__device__ int reduce_scatter_group(const ishmemi_c_device_ctx_t *c, int team, T *dest, const T *source,
                                    size_t nreduce)
{
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS) return 1;  // not initialised / bad handle
    const int tid = G::rank(), nthr = G::size();
    const int size = c->team_size[team], me = c->team_my_idx[team];
    if (size <= 0 || me < 0) return 1;
    uint32_t epoch = 0;
    if (tid == 0)
        epoch = __hip_atomic_fetch_add(c->epochs + team, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    epoch = G::bcast(epoch);
    if (size == 1) {  // one PE: dest = block 0
        if (dest != source)
            for (size_t i = tid; i < nreduce; i += nthr) dest[i] = source[i];
        G::sync();
        return 0;
    }
    if (!group_barrier<G>(c, team, 0, epoch, true)) return 1;
    const int start = c->team_start[team], stride = c->team_stride[team];
    const T *block = source + (size_t) me * nreduce;  // the same offset in every member's heap
    constexpr size_t E = 16 / sizeof(T);
    const bool vec = ((((uintptr_t) dest) | ((uintptr_t) block)) & 15) == 0;
    const size_t nv = vec ? nreduce / E : 0;
    for (size_t v0 = 0; v0 < nv; v0 += (size_t) nthr * kUnroll) {
        Vec16<T> acc[kUnroll];
        for (int j0 = 0; j0 < size; j0 += kMemberBatch) {
            Vec16<T> x[kMemberBatch][kUnroll];
#pragma unroll
            for (int b = 0; b < kMemberBatch; ++b) {
                const int j = j0 + b;
                if (j >= size) break;
                const char *base = (j == me) ? (const char *) block : peer_addr(c, block, start + j * stride);
                const char *step = group_uniform(base + v0 * 16);
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) {
                    const size_t k = (size_t) u * nthr + tid;
                    if (v0 + k < nv) x[b][u] = sys_load16<T>(step, (uint32_t) (k * 16));
                }
            }
#pragma unroll
            for (int b = 0; b < kMemberBatch; ++b) {
                if (j0 + b >= size) break;
#pragma unroll
                for (int u = 0; u < kUnroll; ++u) acc[u] = (j0 + b == 0) ? x[b][u] : op16<T, OP>(acc[u], x[b][u]);
            }
        }
        char *dstep = (char *) group_uniform((const char *) dest + v0 * 16);
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const size_t k = (size_t) u * nthr + tid;
            if (v0 + k < nv) sys_store16<T>(dstep, (uint32_t) (k * 16), acc[u]);
        }
    }
    for (size_t i = nv * E + tid; i < nreduce; i += nthr) {
        T acc = T();
        for (int j = 0; j < size; ++j) {
            const T x = (j == me) ? block[i] : sys_load((const T *) peer_addr(c, block + i, start + j * stride));
            acc = (j == 0) ? x : op1<T, OP>(acc, x);
        }
        sys_store(dest + i, acc);
    }
    return group_barrier<G>(c, team, 2, epoch, false) ? 0 : 1;
}

// ---- fcollect / collect / sum-scan from inside a kernel ------------------------------------
// The reference's ishmemx_<TN>_{fcollect,collect,sum_inscan,sum_exscan}_work_group and their
// device-side blocking forms (src/ishmemx.h, src/collectives/collect_impl.h, scan_impl.h), on the
// reduce's machinery: start barrier (every member's source final, this group's writes released),
// pulls with system-coherent loads into the local dest, end barrier (no member returns while a
// peer may still read its source).

// `nbytes` from `src` (a peer's when `remote`) to the local `dst` by the group: 16-B items when
// both addresses and the length allow, 4-B or single bytes otherwise.
template <typename G>
__device__ inline void group_copy(const char *src, char *dst, size_t nbytes, bool remote)
{
    const int tid = G::rank(), nthr = G::size();
    const uintptr_t al = (uintptr_t) src | (uintptr_t) dst | (uintptr_t) nbytes;
    if ((al & 15) == 0) {
        const size_t nv = nbytes / 16;
        for (size_t v0 = 0; v0 < nv; v0 += (size_t) nthr * kUnroll) {
            const char *step = group_uniform(src + v0 * 16);
            Vec16<uint32_t> x[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const size_t k = (size_t) u * nthr + tid;
                if (v0 + k < nv)
                    x[u] = remote ? sys_load16<uint32_t>(step, (uint32_t) (k * 16)) : ((const Vec16<uint32_t> *) step)[k];
            }
            Vec16<uint32_t> *dp = (Vec16<uint32_t> *) (dst + v0 * 16);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const size_t k = (size_t) u * nthr + tid;
                if (v0 + k < nv) dp[k] = x[u];
            }
        }
    } else if ((al & 3) == 0) {
        for (size_t i = tid; i < nbytes / 4; i += nthr)
            ((uint32_t *) dst)[i] = remote ? sys_load((const uint32_t *) src + i) : ((const uint32_t *) src)[i];
    } else {
        for (size_t i = tid; i < nbytes; i += nthr)
            dst[i] = remote ? (char) sys_load((const uint8_t *) src + i) : src[i];
    }
}

template <typename G>
__device__ inline uint32_t group_epoch(const ishmemi_c_device_ctx_t *c, int team)
{
    uint32_t epoch = 0;
    if (G::rank() == 0)
        epoch = __hip_atomic_fetch_add(c->epochs + team, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    return G::bcast(epoch);
}

// fcollect (equal counts) when counts == nullptr; collect otherwise: this member contributes
// `mybytes`, published in its symmetric count slot before the start barrier and read by every
// member after it (pull: no peer stores into this PE's coarse-grained heap).
template <typename G>
__device__ inline int collect_group(const ishmemi_c_device_ctx_t *c, int team, void *dest, const void *source,
                                    size_t mybytes, bool equal)
{
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS) return 1;  // not initialised / bad handle
    const int size = c->team_size[team], me = c->team_my_idx[team];
    if (size <= 0 || me < 0) return 1;
    const uint32_t epoch = group_epoch<G>(c, team);
    if (size == 1) {
        if (dest != source) group_copy<G>((const char *) source, (char *) dest, mybytes, false);
        G::sync();
        return 0;
    }
    uint64_t *slot = c->dev_counts + (size_t) team * 8;
    if (!equal && G::rank() == 0) sys_store(slot, (uint64_t) mybytes);  // write-through; barrier drains it
    if (!group_barrier<G>(c, team, 0, epoch, true)) return 1;
    const int start = c->team_start[team], stride = c->team_stride[team];
    size_t off = 0;
    for (int j = 0; j < size; ++j) {
        const int gpe = start + j * stride;
        const size_t nb = equal ? mybytes : (size_t) sys_load((const uint64_t *) peer_addr(c, slot, gpe));
        if (nb) {
            const char *src = j == me ? (const char *) source : peer_addr(c, source, gpe);
            group_copy<G>(src, (char *) dest + off, nb, j != me);
        }
        off += nb;
    }
    return group_barrier<G>(c, team, 2, epoch, false) ? 0 : 1;
}

// alltoall (src/collectives/alltoall_impl.h): `nbytes` per block; this member pulls the block
// meant for it (block `me`) out of every member's source into block j of its dest, peers in the
// order me+1, me+2, ..., me (its own block last, a local copy).  Pull, like collect_group: no peer
// stores into this PE's coarse-grained heap.  Same epoch and phase slots as collect_group.  dest
// must not overlap source (a peer may still be reading it).
template <typename G>
__device__ inline int alltoall_group(const ishmemi_c_device_ctx_t *c, int team, void *dest, const void *source,
                                     size_t nbytes)
{
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS) return 1;  // not initialised / bad handle
    const int size = c->team_size[team], me = c->team_my_idx[team];
    if (size <= 0 || me < 0) return 1;
    const uint32_t epoch = group_epoch<G>(c, team);
    if (size == 1) {
        if (dest != source) group_copy<G>((const char *) source, (char *) dest, nbytes, false);
        G::sync();
        return 0;
    }
    // Start: every member's source is final (this group's own writes released).
    if (!group_barrier<G>(c, team, 0, epoch, true)) return 1;
    const int start = c->team_start[team], stride = c->team_stride[team];
    const char *mine = (const char *) source + (size_t) me * nbytes;
    if (nbytes)
        for (int k = 1; k <= size; ++k) {
            const int j = (me + k) % size;
            const char *src = j == me ? mine : peer_addr(c, mine, start + j * stride);
            group_copy<G>(src, (char *) dest + (size_t) j * nbytes, nbytes, j != me);
        }
    // End: no member returns while a peer may still read its source.
    return group_barrier<G>(c, team, 2, epoch, false) ? 0 : 1;
}

// Prefix sum in team order: member me folds members 0..me (inclusive) or 0..me-1 (exclusive;
// member 0 gets 0) element by element — the first term passes through unchanged, as in the host
// scan.  dest must not overlap source (a peer may still be reading it).
template <typename G, typename T>
__device__ inline int scan_group(const ishmemi_c_device_ctx_t *c, int team, T *dest, const T *source,
                                 size_t nelems, bool inclusive)
{
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS) return 1;  // not initialised / bad handle
    const int tid = G::rank(), nthr = G::size();
    const int size = c->team_size[team], me = c->team_my_idx[team];
    // dest and source must be disjoint: a peer may still be reading this PE's source.
    const bool overlap = (const char *) dest < (const char *) (source + nelems) &&
                         (const char *) source < (const char *) (dest + nelems);
    if (size <= 0 || me < 0 || (size > 1 && nelems && overlap)) return 1;
    const uint32_t epoch = group_epoch<G>(c, team);
    if (size > 1 && !group_barrier<G>(c, team, 0, epoch, true)) return 1;
    const int last = inclusive ? me : me - 1;
    const int start = c->team_start[team], stride = c->team_stride[team];
    constexpr size_t E = 16 / sizeof(T);
    const bool vec = ((((uintptr_t) dest) | ((uintptr_t) source)) & 15) == 0;
    const size_t nv = vec ? nelems / E : 0;
    for (size_t v0 = 0; v0 < nv; v0 += (size_t) nthr * kUnroll) {
        Vec16<T> acc[kUnroll] = {};
        for (int k = 0; k <= last; ++k) {
            const char *base = k == me ? (const char *) source : peer_addr(c, source, start + k * stride);
            const char *step = group_uniform(base + v0 * 16);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                const size_t q = (size_t) u * nthr + tid;
                if (v0 + q < nv) {
                    const Vec16<T> x = sys_load16<T>(step, (uint32_t) (q * 16));
                    acc[u] = k == 0 ? x : op16<T, ISHMEMI_OP_SUM>(acc[u], x);
                }
            }
        }
        Vec16<T> *dp = (Vec16<T> *) dest + v0;
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const size_t q = (size_t) u * nthr + tid;
            if (v0 + q < nv) dp[q] = acc[u];
        }
    }
    for (size_t i = nv * E + tid; i < nelems; i += nthr) {
        T acc = T();
        for (int k = 0; k <= last; ++k) {
            const T x = k == me ? source[i] : sys_load((const T *) peer_addr(c, source + i, start + k * stride));
            acc = k == 0 ? x : op1<T, ISHMEMI_OP_SUM>(acc, x);
        }
        dest[i] = acc;
    }
    if (size == 1) {
        G::sync();
        return 0;
    }
    return group_barrier<G>(c, team, 2, epoch, false) ? 0 : 1;
}

// Team barrier from inside a kernel (ishmem_team_sync / sync_all / barrier_all and their
// *_work_group forms, src/collectives/sync_impl.h:30-69): the group's writes are released, then
// every member's group meets on the team's phase-3 row.  The device put / get forms complete
// eagerly (write-through stores, drained before they return), so barrier_all's quiet has nothing
// further to complete beyond the wait and release at the head of group_barrier.
template <typename G>
__device__ inline int team_sync_group(const ishmemi_c_device_ctx_t *c, int team)
{
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS) return 1;
    const int size = c->team_size[team], me = c->team_my_idx[team];
    if (size <= 0 || me < 0) return 1;
    if (size == 1) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        G::sync();
        return 0;
    }
    const uint32_t epoch = group_epoch<G>(c, team);
    return group_barrier<G>(c, team, 3, epoch, true) ? 0 : 1;
}

// Broadcast (src/collectives/broadcast_impl.h, its intra-node pull variant): start barrier (the
// root's source is final), every member including the root pulls `nbytes` of the root's source
// into its dest, end barrier (the root may reuse its source).
template <typename G>
__device__ inline int broadcast_group(const ishmemi_c_device_ctx_t *c, int team, void *dest,
                                      const void *source, size_t nbytes, int root)
{
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS) return 1;
    const int size = c->team_size[team], me = c->team_my_idx[team];
    if (size <= 0 || me < 0 || root < 0 || root >= size) return 1;
    const uint32_t epoch = group_epoch<G>(c, team);
    if (size == 1) {
        if (dest != source) group_copy<G>((const char *) source, (char *) dest, nbytes, false);
        G::sync();
        return 0;
    }
    if (!group_barrier<G>(c, team, 0, epoch, true)) return 1;
    const int groot = c->team_start[team] + root * c->team_stride[team];
    if (root != me) group_copy<G>(peer_addr(c, source, groot), (char *) dest, nbytes, true);
    else if (dest != source) group_copy<G>((const char *) source, (char *) dest, nbytes, false);
    return group_barrier<G>(c, team, 2, epoch, false) ? 0 : 1;
}

// ---- put / get from inside a kernel (src/rma_impl.h:46-75, :116-145) -------------------------
// `nbytes` between this PE's memory and a peer's mapped heap, spread over the group; the layout
// follows the STORE side (head < 16 B up to dst's 16-B boundary, 16-B body, tail), the load side
// is read at the same offsets (unaligned 16-B loads when it sits on another 16-B phase).
//   PUT: plain local loads, remote stores system-coherent write-through (sc0 sc1);
//   GET: remote loads system-coherent (sc0 sc1, never a warm L1 / L2 line), plain local stores.
// A group's threads all pass the same pointers (scalar descriptor base); single work-items may
// each pass their own, so thread_t keeps the base per lane.
template <typename G>
__device__ __forceinline__ const char *rma_base(const char *p)
{
    if constexpr (std::is_same_v<G, thread_t>) return p;
    else return group_uniform(p);
}

template <typename G, bool PUT>
__device__ inline void rma_group(char *dst, const char *src, size_t nbytes)
{
    const int tid = G::rank(), nthr = G::size();
    size_t head = (16 - ((uintptr_t) dst & 15)) & 15;
    if (head > nbytes) head = nbytes;
    const size_t nv = (nbytes - head) / 16, tail = nbytes - head - nv * 16;
    const char *sb = src + head;
    char *db = dst + head;
    for (size_t v0 = 0; v0 < nv; v0 += (size_t) nthr * kUnroll) {
        const char *ls = rma_base<G>(sb + v0 * 16);
        char *ds = (char *) rma_base<G>(db + v0 * 16);
        const __amdgpu_buffer_rsrc_t lr =
            __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(ls), (short) 0, 0x7FFFFFFF, 0x00020000);
        Vec16<uint32_t> x[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const size_t k = (size_t) u * nthr + tid;
            if (v0 + k < nv)
                x[u] = __builtin_bit_cast(Vec16<uint32_t>,
                                          __builtin_amdgcn_raw_buffer_load_b128(lr, (uint32_t) (k * 16), 0, PUT ? 0 : 17));
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const size_t k = (size_t) u * nthr + tid;
            if (v0 + k >= nv) continue;
            if constexpr (PUT) sys_store16<uint32_t>(ds, (uint32_t) (k * 16), x[u]);
            else ((Vec16<uint32_t> *) ds)[k] = x[u];
        }
    }
    for (size_t i = tid; i < head + tail; i += nthr) {
        const size_t off = i < head ? i : nv * 16 + i;
        if constexpr (PUT) sys_store((uint8_t *) dst + off, ((const uint8_t *) src)[off]);
        else dst[off] = (char) sys_load((const uint8_t *) src + off);
    }
}

// Blocking put / get by the group G (thread_t: one work-item): group sync, the copy, every
// thread's accesses drained (a write-through store counts as done once memory has it), group sync.
// The _nbi device forms are the same call: they complete eagerly.
template <typename G, bool PUT>
__device__ inline void rma_call(void *dest, const void *source, size_t nbytes, int pe)
{
    const ishmemi_c_device_ctx_t *c = ctx();
    if (!c || pe < 0 || pe >= c->npes) return;
    G::sync();
    if (nbytes) {
        if constexpr (PUT) rma_group<G, true>(peer_addr(c, dest, pe), (const char *) source, nbytes);
        else rma_group<G, false>((char *) dest, peer_addr(c, source, pe), nbytes);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G::sync();
}

// ---- strided / blocked put / get from inside a kernel (src/ishmem/copy.h:184-219, :389-427) -----
// nblocks blocks of bsize elements of ES bytes, block b from src + b * sst to dst + b * dst_stride
// (element strides), spread over the group.  The item is the host kernel's: the
// largest power of two <= 16 dividing both addresses, the block's byte length and, for more than one
// block, both byte strides, so every access is naturally aligned.  Consecutive threads take
// consecutive items of a block, then the next block's.  Every address is a per-thread 64-bit pointer
// (base + b * stride + w * W in 64 bits): nothing to wrap however far the extent reaches.
//   PUT: plain local loads, remote stores system-coherent write-through (sc0 sc1);
//   GET: remote loads system-coherent (sc0 sc1), plain local stores.
template <int W>
struct strided_item {
    using type = std::conditional_t<W == 8, uint64_t, std::conditional_t<W == 4, uint32_t,
                 std::conditional_t<W == 2, uint16_t, uint8_t>>>;
};
template <>
struct strided_item<16> {
    typedef unsigned type __attribute__((ext_vector_type(4)));
};

template <typename I>
__device__ __forceinline__ I sys_item_load(const char *p)
{
    if constexpr (sizeof(I) == 16) return __builtin_amdgcn_global_load_b128((__attribute__((address_space(1))) I *) p, "");
    else return sys_load((const I *) p);
}

template <typename I>
__device__ __forceinline__ void sys_item_store(char *p, const I &v)
{
    if constexpr (sizeof(I) == 16) __builtin_amdgcn_global_store_b128((__attribute__((address_space(1))) I *) p, v, "");
    else sys_store((I *) p, v);
}

template <typename G, bool PUT, int W>
__device__ inline void rma_strided_items(char *dst, const char *src, uint64_t dstride, uint64_t sstride, uint64_t ipb,
                                         uint64_t nblocks)
{
    using I = typename strided_item<W>::type;
    const uint64_t nthr = (uint64_t) G::size(), nitems = nblocks * ipb;
    // One division per thread per call; then step nthr items at a time.
    const uint64_t step_b = nthr / ipb, step_w = nthr - step_b * ipb;
    uint64_t b = (uint64_t) G::rank() / ipb, w = (uint64_t) G::rank() - b * ipb;
    for (uint64_t g0 = (uint64_t) G::rank(); g0 < nitems; g0 += nthr * kUnroll) {
        I x[kUnroll];
        char *dp[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            // Threads past the end load item 0 again (and store nothing): no branch round a load, so all
            // kUnroll loads are in flight before the first store.
            const char *sp = g0 + (uint64_t) u * nthr < nitems ? src + b * sstride + w * W : src;
            dp[u] = dst + b * dstride + w * W;
            if constexpr (PUT) x[u] = *(const I *) sp;
            else x[u] = sys_item_load<I>(sp);
            b += step_b;
            w += step_w;
            if (w >= ipb) {
                w -= ipb;
                ++b;
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (g0 + (uint64_t) u * nthr >= nitems) continue;
            if constexpr (PUT) sys_item_store<I>(dp[u], x[u]);
            else *(I *) dp[u] = x[u];
        }
    }
}

// Not inlined: the five item widths are compiled once per group kind and direction, not once per
// call site of the few hundred names below.
template <typename G, bool PUT>
__device__ __attribute__((noinline)) void rma_strided_group(char *dst, const char *src, uint64_t dstride, uint64_t sstride, uint64_t block_bytes,
                                         uint64_t nblocks)
{
    uint64_t bits = (uint64_t) dst | (uint64_t) src | block_bytes | 16;
    if (nblocks > 1) bits |= dstride | sstride;
    const uint64_t wd = bits & (~bits + 1), ipb = block_bytes / wd;
    switch (wd) {
        case 16: rma_strided_items<G, PUT, 16>(dst, src, dstride, sstride, ipb, nblocks); break;
        case 8: rma_strided_items<G, PUT, 8>(dst, src, dstride, sstride, ipb, nblocks); break;
        case 4: rma_strided_items<G, PUT, 4>(dst, src, dstride, sstride, ipb, nblocks); break;
        case 2: rma_strided_items<G, PUT, 2>(dst, src, dstride, sstride, ipb, nblocks); break;
        default: rma_strided_items<G, PUT, 1>(dst, src, dstride, sstride, ipb, nblocks); break;
    }
}

// Blocking strided / blocked put / get by the group G: the sync, drain, sync bracket of rma_call.
// Strides < 1 or < bsize are an argument error (device error word, nothing moved).
template <typename G, bool PUT>
__device__ inline void rma_strided_call(void *dest, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t bsize,
                                        size_t nblocks, size_t elem_bytes, int pe)
{
    const ishmemi_c_device_ctx_t *c = ctx();
    if (!c || pe < 0 || pe >= c->npes) return;
    if (dst < 1 || sst < 1 || (size_t) dst < bsize || (size_t) sst < bsize) {
        if (G::rank() == 0)  // kErrBadArgument
            __hip_atomic_fetch_or(c->err, 1u << 9, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    G::sync();
    if (nblocks && bsize) {
        if constexpr (PUT)
            rma_strided_group<G, true>(peer_addr(c, dest, pe), (const char *) source, (uint64_t) dst * elem_bytes,
                                       (uint64_t) sst * elem_bytes, (uint64_t) bsize * elem_bytes, nblocks);
        else
            rma_strided_group<G, false>((char *) dest, peer_addr(c, source, pe), (uint64_t) dst * elem_bytes,
                                        (uint64_t) sst * elem_bytes, (uint64_t) bsize * elem_bytes, nblocks);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G::sync();
}

// quiet / fence: the calling thread's outstanding memory operations, then a system-scope release
// (the second wait is kept: the fence's own may be dropped by the compiler).
template <typename G>
__device__ inline void quiet_group()
{
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G::sync();
    if (G::rank() == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    G::sync();
}

// ---- put with signal, wait_until / test from inside a kernel ------------------
// Bits of the device-API error word (c->err) beside the barrier phases' bits 0-3.
constexpr uint32_t kErrWaitTimeout = 1u << 8, kErrBadArgument = 1u << 9;

__device__ __forceinline__ void record_error(const ishmemi_c_device_ctx_t *c, uint32_t bit)
{
    __hip_atomic_fetch_or(c->err, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The payload as rma_call<G, true> moves it; EVERY lane then waits for its stores (write-through:
// acknowledged once the target's memory has them), the group meets, and only then the leader updates
// the signal word on the target with one system-scope atomic; the group meets again, so no lane
// returns before the signal is issued.
template <typename G>
__device__ inline void put_signal_call(void *dest, const void *source, size_t nbytes, uint64_t *sig_addr, uint64_t signal,
                                       int sig_op, int pe)
{
    const ishmemi_c_device_ctx_t *c = ctx();
    if (!c || pe < 0 || pe >= c->npes) return;
    if (sig_op != ISHMEMI_C_SIGNAL_SET && sig_op != ISHMEMI_C_SIGNAL_ADD) {
        if (G::rank() == 0) record_error(c, kErrBadArgument);
        return;
    }
    G::sync();
    if (nbytes) rma_group<G, true>(peer_addr(c, dest, pe), (const char *) source, nbytes);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    G::sync();
    if (G::rank() == 0) {
        uint64_t *rsig = (uint64_t *) peer_addr(c, sig_addr, pe);
        if (sig_op == ISHMEMI_C_SIGNAL_ADD)
            (void) __hip_atomic_fetch_add(rsig, signal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else __hip_atomic_store(rsig, signal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    G::sync();
}

__device__ inline void signal_op_call(uint64_t *sig_addr, uint64_t signal, int sig_op, int pe)
{
    const ishmemi_c_device_ctx_t *c = ctx();
    if (!c || pe < 0 || pe >= c->npes) return;
    uint64_t *rsig = (uint64_t *) peer_addr(c, sig_addr, pe);
    if (sig_op == ISHMEMI_C_SIGNAL_ADD) (void) __hip_atomic_fetch_add(rsig, signal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    else __hip_atomic_store(rsig, signal, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// ISHMEM_CMP_* in the variable's own type.
template <typename T>
__device__ __forceinline__ bool sync_compare(T v, int cmp, T c)
{
    switch (cmp) {
        case ISHMEMI_C_CMP_EQ: return v == c;
        case ISHMEMI_C_CMP_NE: return v != c;
        case ISHMEMI_C_CMP_GT: return v > c;
        case ISHMEMI_C_CMP_GE: return v >= c;
        case ISHMEMI_C_CMP_LT: return v < c;
        default: return v <= c;
    }
}

// wait_until (budget 0) / test (budget 1) by the group G.  The leader polls the variable relaxed at
// system scope with a bounded back-off (s_sleep 1 for 32 polls, then 8; the clock every 16 polls).
// After the match ONE system-scope acquire, and the leader waits for its invalidate BEFORE the
// group's barrier inside bcast (as group_barrier does), so every wave's plain loads of the bytes the
// signal announces land behind it.  Returns the value read; *matched = 1 / 0.  A timeout or an
// invalid cmp is recorded in the device-API error word and returns with *matched = 0.
template <typename G, typename T>
__device__ inline T wait_until_group(T *ivar, int cmp, T cmp_value, uint32_t budget, int *matched)
{
    static_assert(std::is_integral_v<T> && (sizeof(T) == 4 || sizeof(T) == 8), "wait_until / test: 32- or 64-bit integers");
    using U = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>;
    const ishmemi_c_device_ctx_t *c = ctx();
    uint64_t bits = 0;
    uint32_t ok = 0;
    if (c && G::rank() == 0) {
        if (cmp < ISHMEMI_C_CMP_EQ || cmp > ISHMEMI_C_CMP_LE) {
            record_error(c, kErrBadArgument);
        } else {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            for (uint32_t it = 0;; ++it) {
                const U u = __hip_atomic_load((const U *) ivar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                bits = u;
                if (sync_compare<T>((T) u, cmp, cmp_value)) {
                    ok = 1;
                    break;
                }
                if (budget && it + 1 >= budget) break;
                if ((it & 15) == 15 && __builtin_amdgcn_s_memrealtime() - t0 > c->timeout_ticks) {
                    record_error(c, kErrWaitTimeout);
                    break;
                }
                if (it < 32) __builtin_amdgcn_s_sleep(1);
                else __builtin_amdgcn_s_sleep(8);
            }
            if (ok) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
        }
    }
    if constexpr (!std::is_same_v<G, thread_t>) {
        const uint32_t lo = G::bcast((uint32_t) bits), hi = sizeof(T) == 8 ? G::bcast((uint32_t) (bits >> 32)) : 0u;
        bits = ((uint64_t) hi << 32) | lo;
        ok = G::bcast(ok);
    }
    if (matched) *matched = (int) ok;
    return (T) (U) bits;
}

// ---- vector waits and tests from inside a kernel -------------------------------
// wait_until_all / any / some and test_all / any / some (mode: ISHMEMI_C_SYNC_*, with ISHMEMI_C_SYNC_VECTOR
// for the per-element compare values) by the group G.  Polls are relaxed system-scope loads of the
// variable's own width with wait_until_group's back-off and clock check; a test is one pass.
// Returns all: 1 / 0, any: the index or SIZE_MAX, some: the count.  *st = 0 matched (an empty wait set
// included), 1 timed out, 2 a test that found nothing.
constexpr int kSyncVec = ISHMEMI_C_SYNC_VECTOR;
constexpr uint32_t kSyncMatched = 0, kSyncTimedOut = 1, kSyncNoMatch = 2;

template <typename T>
__device__ __forceinline__ bool sync_poll_compare(const T *ivars, size_t i, int cmp, T cv)
{
    using U = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>;
    const U u = __hip_atomic_load((const U *) ivars + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return sync_compare<T>((T) u, cmp, cv);
}

__device__ __forceinline__ bool sync_give_up(const ishmemi_c_device_ctx_t *c, uint32_t it, uint64_t t0)
{
    return (it & 15) == 15 && __builtin_amdgcn_s_memrealtime() - t0 > c->timeout_ticks;
}

__device__ __forceinline__ void sync_backoff(uint32_t it)
{
    if (it < 32) __builtin_amdgcn_s_sleep(1);
    else __builtin_amdgcn_s_sleep(8);
}

// One lane sweeps the elements itself: no cross-lane operation, so divergent callers are legal.
template <typename T>
__device__ inline uint64_t sync_sweep_lane(const ishmemi_c_device_ctx_t *c, int mode, const T *ivars, size_t nelems,
                                           size_t *indices, const int *status, int cmp, T cmp_value, const T *cmp_values,
                                           uint32_t *st)
{
    const bool test = mode >= ISHMEMI_C_SYNC_TEST_ALL;
    const int kind = test ? mode - ISHMEMI_C_SYNC_TEST_ALL : mode;  // 0 all, 1 any, 2 some
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    uint32_t it = 0;
    *st = kSyncMatched;
    if (kind == 0) {
        // In order, each element until it was seen satisfied once; it is not read again.
        for (size_t i = 0; i < nelems; ++i) {
            if (status && status[i]) continue;
            const T cv = cmp_values ? cmp_values[i] : cmp_value;
            for (;; ++it) {
                if (sync_poll_compare<T>(ivars, i, cmp, cv)) break;
                if (test) return *st = kSyncNoMatch, 0;
                if (sync_give_up(c, it, t0)) return *st = kSyncTimedOut, 0;
                sync_backoff(it);
            }
        }
        return 1;
    }
    size_t start = 0;
    if (kind == 1 && nelems) {
        const uint64_t r = __hip_atomic_load(c->sync_rotor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        start = (size_t) ((r % nelems + 1) % nelems);
    }
    for (;; ++it) {
        size_t count = 0, valid = 0;
        for (size_t k = 0; k < nelems; ++k) {
            const size_t i = start + k < nelems ? start + k : start + k - nelems;
            if (status && status[i]) continue;
            ++valid;
            if (!sync_poll_compare<T>(ivars, i, cmp, cmp_values ? cmp_values[i] : cmp_value)) continue;
            if (kind == 1) return i;
            indices[count++] = i;
        }
        if (count) return count;
        if (valid == 0) return kind == 1 ? (uint64_t) SIZE_MAX : 0;  // empty wait set
        if (test) return *st = kSyncNoMatch, kind == 1 ? (uint64_t) SIZE_MAX : 0;
        if (sync_give_up(c, it, t0)) return *st = kSyncTimedOut, kind == 1 ? (uint64_t) SIZE_MAX : 0;
        sync_backoff(it);
    }
}

// The 64 lanes of one full wave sweep together, one element per lane per sub-pass; every decision
// that ends or continues a loop comes from a ballot or __all and is the same in all lanes.
template <typename T>
__device__ inline uint64_t sync_sweep_wave(const ishmemi_c_device_ctx_t *c, int mode, const T *ivars, size_t nelems,
                                           size_t *indices, const int *status, int cmp, T cmp_value, const T *cmp_values,
                                           uint32_t *st)
{
    const bool test = mode >= ISHMEMI_C_SYNC_TEST_ALL;
    const int kind = test ? mode - ISHMEMI_C_SYNC_TEST_ALL : mode;
    const uint32_t lane = __lane_id();
    const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
    constexpr uint64_t kNone = ~0ull;
    uint32_t it = 0;
    *st = kSyncMatched;
    if (kind == 0) {
        for (size_t base = 0; base < nelems; base += 64) {
            const size_t i = base + lane;
            bool left = i < nelems && !(status && status[i]);
            const T cv = left && cmp_values ? cmp_values[i] : cmp_value;
            for (;; ++it) {
                if (left && sync_poll_compare<T>(ivars, i, cmp, cv)) left = false;
                if (__all(!left)) break;
                if (test) return *st = kSyncNoMatch, 0;
                if (sync_give_up(c, it, t0)) return *st = kSyncTimedOut, 0;
                sync_backoff(it);
            }
        }
        return 1;
    }
    uint64_t start = 0;
    if (kind == 1 && nelems) {
        const uint64_t r = __hip_atomic_load(c->sync_rotor, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        start = (r % nelems + 1) % nelems;
    }
    for (;; ++it) {
        uint64_t count = 0, best_hi = kNone, best_lo = kNone;
        bool nonempty = false;
        for (size_t base = 0; base < nelems; base += 64) {
            const size_t i = base + lane;
            const bool ok = i < nelems && !(status && status[i]);
            const bool match = ok && sync_poll_compare<T>(ivars, i, cmp, cmp_values ? cmp_values[i] : cmp_value);
            const uint64_t m = __ballot(match);
            nonempty |= __ballot(ok) != 0;
            if (m == 0) continue;
            if (kind == 1) {
                if (best_lo == kNone) best_lo = base + (uint64_t) __builtin_ctzll(m);
                uint64_t mh = m;  // the matches at or after `start`
                if (start > base) mh = start - base >= 64 ? 0 : m & (~0ull << (start - base));
                if (mh) {
                    best_hi = base + (uint64_t) __builtin_ctzll(mh);
                    break;
                }
            } else {
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0));
                if (match) indices[count + before] = i;
                count += (uint64_t) __builtin_popcountll(m);
            }
        }
        if (kind == 1 && (best_hi != kNone || best_lo != kNone)) return best_hi != kNone ? best_hi : best_lo;
        if (kind == 2 && count) return count;
        const uint64_t none = kind == 1 ? (uint64_t) SIZE_MAX : 0;
        if (!nonempty) return none;  // empty wait set
        if (test) return *st = kSyncNoMatch, none;
        if (sync_give_up(c, it, t0)) return *st = kSyncTimedOut, none;
        sync_backoff(it);
    }
}

// A group of at least one full wave: its first 64 ranks sweep together, the other waves do not poll
// and meet the sweepers at the group's barrier inside bcast.  A smaller group: the leader sweeps.
// After a match ONE system-scope acquire, and the sweepers wait for its invalidate BEFORE the
// broadcast (as wait_until_group does), so every member's plain loads of what the variables announce,
// and of indices[0 .. count), land behind it.  Every member returns the same value.
template <typename G, typename T>
__device__ inline size_t sync_vector_group(int mode_bits, T *ivars, size_t nelems, size_t *indices, const int *status, int cmp,
                                           T cmp_value, const T *cmp_values)
{
    static_assert(std::is_integral_v<T> && (sizeof(T) == 4 || sizeof(T) == 8), "vector waits / tests: 32- or 64-bit integers");
    const ishmemi_c_device_ctx_t *c = ctx();
    const int mode = mode_bits & ~kSyncVec;
    const bool any = mode == ISHMEMI_C_SYNC_WAIT_ANY || mode == ISHMEMI_C_SYNC_TEST_ANY;
    const bool some = mode == ISHMEMI_C_SYNC_WAIT_SOME || mode == ISHMEMI_C_SYNC_TEST_SOME;
    uint64_t result = any ? (uint64_t) SIZE_MAX : 0;
    if (!c) return (size_t) result;
    if (nelems == 0) return (size_t) (any || some ? result : 1);  // the empty wait set
    if (cmp < ISHMEMI_C_CMP_EQ || cmp > ISHMEMI_C_CMP_LE || !ivars || (some && !indices) ||
        ((mode_bits & kSyncVec) && !cmp_values)) {
        if (G::rank() == 0) record_error(c, kErrBadArgument);
        return (size_t) result;
    }
    const bool wave = !std::is_same_v<G, thread_t> && G::size() >= 64;
    if (wave ? G::rank() < 64 : G::rank() == 0) {
        uint32_t st = kSyncMatched;
        result = wave ? sync_sweep_wave<T>(c, mode, ivars, nelems, indices, status, cmp, cmp_value, cmp_values, &st)
                      : sync_sweep_lane<T>(c, mode, ivars, nelems, indices, status, cmp, cmp_value, cmp_values, &st);
        if (st == kSyncMatched && result != (any ? (uint64_t) SIZE_MAX : 0)) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        if (G::rank() == 0) {
            if (st == kSyncTimedOut) record_error(c, kErrWaitTimeout);
            if (any && result != (uint64_t) SIZE_MAX)
                __hip_atomic_store(c->sync_rotor, result, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if constexpr (!std::is_same_v<G, thread_t>) {
        const uint32_t lo = G::bcast((uint32_t) result), hi = G::bcast((uint32_t) (result >> 32));
        result = ((uint64_t) hi << 32) | lo;
    }
    return (size_t) result;
}

// The one work-item form under the name the shared generator (ishmem_sync.h) calls.
template <typename T>
__device__ inline size_t sync_vector(int mode_bits, T *ivars, size_t nelems, size_t *indices, const int *status, int cmp,
                                     T cmp_value, const T *cmp_values)
{
    return sync_vector_group<thread_t, T>(mode_bits, ivars, nelems, indices, status, cmp, cmp_value, cmp_values);
}

template <typename T>
constexpr bool is_canon()
{
    return std::is_arithmetic_v<T> && sizeof(T) <= 8;
}

}  // namespace ishmemx_dev

/* ---- library queries from a kernel (src/ishmem.h:54-58, :74-77: host and device) ------------ */
__device__ inline int ishmem_my_pe(void)
{
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    return c ? c->pe : -1;
}
__device__ inline int ishmem_n_pes(void)
{
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    return c ? c->npes : -1;
}
__device__ inline void *ishmem_ptr(const void *dest, int pe)
{
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    if (!c || pe < 0 || pe >= c->npes) return nullptr;
    const uint64_t off = (uint64_t) ((const char *) dest - c->heap_base);
    return off < c->heap_size ? (void *) (c->peer_heap[pe] + off) : nullptr;
}
__device__ inline int ishmem_team_my_pe(int team)
{
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS || c->team_size[team] <= 0) return -1;
    return c->team_my_idx[team];
}
__device__ inline int ishmem_team_n_pes(int team)
{
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    if (!c || team < 0 || team >= ISHMEMI_C_MAX_TEAMS || c->team_size[team] <= 0) return -1;
    return c->team_size[team];
}
__device__ inline int ishmem_team_translate_pe(int src_team, int src_pe, int dest_team)
{
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    if (!c || src_team < 0 || src_team >= ISHMEMI_C_MAX_TEAMS || dest_team < 0 ||
        dest_team >= ISHMEMI_C_MAX_TEAMS || c->team_size[src_team] <= 0 || c->team_size[dest_team] <= 0 ||
        src_pe < 0 || src_pe >= c->team_size[src_team])
        return -1;
    const int d = c->team_start[src_team] + src_pe * c->team_stride[src_team] - c->team_start[dest_team];
    const int st = c->team_stride[dest_team];
    if (st == 0 || d % st) return -1;
    return (d / st >= 0 && d / st < c->team_size[dest_team]) ? d / st : -1;
}
__device__ inline void ishmem_info_get_version(int *major, int *minor)
{
    *major = ISHMEMI_C_SPEC_MAJOR;
    *minor = ISHMEMI_C_SPEC_MINOR;
}
__device__ inline void ishmem_info_get_name(char *name)
{
    const char *v = ISHMEMI_C_VENDOR_STRING;
    while (*v) *name++ = *v++;
    *name = '\0';
}

/* ---- synchronisation from a kernel (src/ishmem.h:1555-1559, src/ishmemx.h:2228-2239) -------- */
__device__ inline void ishmem_barrier_all(void)
{
    (void) ishmemx_dev::team_sync_group<ishmemx_dev::thread_t>(ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD);
}
__device__ inline void ishmem_sync_all(void)
{
    (void) ishmemx_dev::team_sync_group<ishmemx_dev::thread_t>(ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD);
}
__device__ inline int ishmem_team_sync(int team)
{
    return ishmemx_dev::team_sync_group<ishmemx_dev::thread_t>(ishmemx_dev::ctx(), team);
}
template <typename Group>
__device__ inline void ishmemx_barrier_all_work_group(const Group &)
{
    (void) ishmemx_dev::team_sync_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD);
}
template <typename Group>
__device__ inline void ishmemx_sync_all_work_group(const Group &)
{
    (void) ishmemx_dev::team_sync_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD);
}
template <typename Group>
__device__ inline void ishmemx_team_sync_work_group(int team, const Group &)
{
    (void) ishmemx_dev::team_sync_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team);
}

/* ---- device print (src/ishmemx.h:2256-2271; the reference sends it to a host proxy thread, a
 *      HIP kernel prints directly) --------------------------------------------------------------- */
typedef enum { DEBUG, WARNING, ERROR, STDOUT, STDERR } ishmemx_print_msg_type_t;
__device__ inline void ishmemx_print(const char *file, long int line, const char *func, const char *out,
                                     ishmemx_print_msg_type_t msg_type)
{
    const char *kind = msg_type == DEBUG ? "DEBUG" : msg_type == WARNING ? "WARN" : msg_type == ERROR ? "ERROR" : "";
    if (file) printf("[%d] %s %s:%ld %s: %s", ishmem_my_pe(), kind, file, line, func ? func : "", out);
    else printf("[%d] %s%s%s", ishmem_my_pe(), kind, *kind ? ": " : "", out);
}
__device__ inline void ishmemx_print(const char *out, ishmemx_print_msg_type_t msg_type)
{
    ishmemx_print(nullptr, 0, nullptr, out, msg_type);
}
__device__ inline void ishmemx_print(const char *out) { ishmemx_print(nullptr, 0, nullptr, out, DEBUG); }

/* ---- reductions ------------------------------------------------------------------------------ */
#define ISHMEMX_DEV_GENERIC(OPNAME, OPC)                                                           \
    template <typename T, typename Group>                                                          \
    __device__ inline int ishmemx_##OPNAME##_reduce_work_group(T *dest, const T *source,           \
                                                               size_t nreduce, const Group &)      \
    {                                                                                              \
        return ishmemx_dev::reduce_group<ishmemx_dev::exec_t<Group>, T, OPC>(                      \
            ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD, dest, source, nreduce);                      \
    }                                                                                              \
    template <typename T, typename Group>                                                          \
    __device__ inline int ishmemx_##OPNAME##_reduce_work_group(int team, T *dest, const T *source, \
                                                               size_t nreduce, const Group &)      \
    {                                                                                              \
        return ishmemx_dev::reduce_group<ishmemx_dev::exec_t<Group>, T, OPC>(ishmemx_dev::ctx(),   \
                                                                             team, dest, source,   \
                                                                             nreduce);             \
    }                                                                                              \
    template <typename T>                                                                          \
    __device__ inline int ishmem_##OPNAME##_reduce(T *dest, const T *source, size_t nreduce)       \
    {                                                                                              \
        return ishmemx_dev::reduce_group<ishmemx_dev::thread_t, T, OPC>(                           \
            ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD, dest, source, nreduce);                      \
    }                                                                                              \
    template <typename T>                                                                          \
    __device__ inline int ishmem_##OPNAME##_reduce(int team, T *dest, const T *source,             \
                                                   size_t nreduce)                                 \
    {                                                                                              \
        return ishmemx_dev::reduce_group<ishmemx_dev::thread_t, T, OPC>(ishmemx_dev::ctx(), team,  \
                                                                        dest, source, nreduce);    \
    }

ISHMEMX_DEV_GENERIC(and, ISHMEMI_OP_AND)
ISHMEMX_DEV_GENERIC(or, ISHMEMI_OP_OR)
ISHMEMX_DEV_GENERIC(xor, ISHMEMI_OP_XOR)
ISHMEMX_DEV_GENERIC(max, ISHMEMI_OP_MAX)
ISHMEMX_DEV_GENERIC(min, ISHMEMI_OP_MIN)
ISHMEMX_DEV_GENERIC(sum, ISHMEMI_OP_SUM)
ISHMEMX_DEV_GENERIC(prod, ISHMEMI_OP_PROD)

#define ISHMEMX_DEV_TYPED(TYPENAME, TYPE, OPNAME, OPC)                                              \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_work_group(                       \
        TYPE *dest, const TYPE *source, size_t nreduce, const Group &grp)                          \
    {                                                                                              \
        return ishmemx_##OPNAME##_reduce_work_group<TYPE>(dest, source, nreduce, grp);             \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_work_group(                       \
        int team, TYPE *dest, const TYPE *source, size_t nreduce, const Group &grp)                \
    {                                                                                              \
        return ishmemx_##OPNAME##_reduce_work_group<TYPE>(team, dest, source, nreduce, grp);       \
    }                                                                                              \
    __device__ inline int ishmem_##TYPENAME##_##OPNAME##_reduce(TYPE *dest, const TYPE *source,    \
                                                                size_t nreduce)                    \
    {                                                                                              \
        return ishmem_##OPNAME##_reduce<TYPE>(dest, source, nreduce);                              \
    }                                                                                              \
    __device__ inline int ishmem_##TYPENAME##_##OPNAME##_reduce(int team, TYPE *dest,              \
                                                                const TYPE *source, size_t nreduce) \
    {                                                                                              \
        return ishmem_##OPNAME##_reduce<TYPE>(team, dest, source, nreduce);                        \
    }

/* ---- reduce-scatter (extension; ishmemx.h has the semantics, DESIGN.md §3h the design) ---------
 *   ishmemx_<TN>_<op>_reduce_scatter_work_group([team,] dest, source, nreduce, grp)
 *   ishmemx_<TN>_<op>_reduce_scatter([team,] dest, source, nreduce)            (one work-item)
 * and the generic ishmemx_<op>_reduce_scatter_work_group<T> / ishmemx_<op>_reduce_scatter<T>.
 * dest overlapping source is undefined here (the host forms refuse it). */
#define ISHMEMX_DEV_RS_GENERIC(OPNAME, OPC)                                                         \
    template <typename T, typename Group>                                                          \
    __device__ inline int ishmemx_##OPNAME##_reduce_scatter_work_group(T *dest, const T *source,   \
                                                                       size_t nreduce, const Group &) \
    {                                                                                              \
        return ishmemx_dev::reduce_scatter_group<ishmemx_dev::exec_t<Group>, T, OPC>(              \
            ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD, dest, source, nreduce);                      \
    }                                                                                              \
    template <typename T, typename Group>                                                          \
    __device__ inline int ishmemx_##OPNAME##_reduce_scatter_work_group(int team, T *dest,          \
                                                                       const T *source,            \
                                                                       size_t nreduce, const Group &) \
    {                                                                                              \
        return ishmemx_dev::reduce_scatter_group<ishmemx_dev::exec_t<Group>, T, OPC>(              \
            ishmemx_dev::ctx(), team, dest, source, nreduce);                                      \
    }                                                                                              \
    template <typename T>                                                                          \
    __device__ inline int ishmemx_##OPNAME##_reduce_scatter(T *dest, const T *source, size_t nreduce) \
    {                                                                                              \
        return ishmemx_dev::reduce_scatter_group<ishmemx_dev::thread_t, T, OPC>(                   \
            ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD, dest, source, nreduce);                      \
    }                                                                                              \
    template <typename T>                                                                          \
    __device__ inline int ishmemx_##OPNAME##_reduce_scatter(int team, T *dest, const T *source,    \
                                                            size_t nreduce)                        \
    {                                                                                              \
        return ishmemx_dev::reduce_scatter_group<ishmemx_dev::thread_t, T, OPC>(ishmemx_dev::ctx(), team, \
                                                                                dest, source, nreduce); \
    }

ISHMEMX_DEV_RS_GENERIC(and, ISHMEMI_OP_AND)
ISHMEMX_DEV_RS_GENERIC(or, ISHMEMI_OP_OR)
ISHMEMX_DEV_RS_GENERIC(xor, ISHMEMI_OP_XOR)
ISHMEMX_DEV_RS_GENERIC(max, ISHMEMI_OP_MAX)
ISHMEMX_DEV_RS_GENERIC(min, ISHMEMI_OP_MIN)
ISHMEMX_DEV_RS_GENERIC(sum, ISHMEMI_OP_SUM)
ISHMEMX_DEV_RS_GENERIC(prod, ISHMEMI_OP_PROD)

#define ISHMEMX_DEV_RS_TYPED(TYPENAME, TYPE, OPNAME, OPC)                                           \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_scatter_work_group(               \
        TYPE *dest, const TYPE *source, size_t nreduce, const Group &grp)                          \
    {                                                                                              \
        return ishmemx_##OPNAME##_reduce_scatter_work_group<TYPE>(dest, source, nreduce, grp);     \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_scatter_work_group(               \
        int team, TYPE *dest, const TYPE *source, size_t nreduce, const Group &grp)                \
    {                                                                                              \
        return ishmemx_##OPNAME##_reduce_scatter_work_group<TYPE>(team, dest, source, nreduce, grp); \
    }                                                                                              \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_scatter(TYPE *dest, const TYPE *source, \
                                                                         size_t nreduce)           \
    {                                                                                              \
        return ishmemx_dev::reduce_scatter_group<ishmemx_dev::thread_t, TYPE, OPC>(                \
            ishmemx_dev::ctx(), ISHMEMI_C_TEAM_WORLD, dest, source, nreduce);                      \
    }                                                                                              \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_scatter(int team, TYPE *dest,     \
                                                                         const TYPE *source,       \
                                                                         size_t nreduce)           \
    {                                                                                              \
        return ishmemx_dev::reduce_scatter_group<ishmemx_dev::thread_t, TYPE, OPC>(ishmemx_dev::ctx(), team, \
                                                                                   dest, source, nreduce); \
    }

/* ---- fcollect / collect / sum_inscan / sum_exscan / broadcast --------------------------------- */
template <typename T, typename Group>
__device__ inline int ishmemx_fcollect_work_group(int team, T *dest, const T *source, size_t nelems, const Group &)
{
    return ishmemx_dev::collect_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source,
                                                                  nelems * sizeof(T), true);
}
template <typename T, typename Group>
__device__ inline int ishmemx_collect_work_group(int team, T *dest, const T *source, size_t nelems, const Group &)
{
    return ishmemx_dev::collect_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source,
                                                                  nelems * sizeof(T), false);
}
template <typename T, typename Group>
__device__ inline int ishmemx_alltoall_work_group(int team, T *dest, const T *source, size_t nelems, const Group &)
{
    return ishmemx_dev::alltoall_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source,
                                                                   nelems * sizeof(T));
}
template <typename T, typename Group>
__device__ inline int ishmemx_sum_inscan_work_group(int team, T *dest, const T *source, size_t nelems, const Group &)
{
    return ishmemx_dev::scan_group<ishmemx_dev::exec_t<Group>, T>(ishmemx_dev::ctx(), team, dest, source, nelems,
                                                                  true);
}
template <typename T, typename Group>
__device__ inline int ishmemx_sum_exscan_work_group(int team, T *dest, const T *source, size_t nelems, const Group &)
{
    return ishmemx_dev::scan_group<ishmemx_dev::exec_t<Group>, T>(ishmemx_dev::ctx(), team, dest, source, nelems,
                                                                  false);
}
template <typename T, typename Group>
__device__ inline int ishmemx_broadcast_work_group(int team, T *dest, const T *source, size_t nelems, int root,
                                                   const Group &)
{
    return ishmemx_dev::broadcast_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source,
                                                                    nelems * sizeof(T), root);
}
#define ISHMEMX_DEV_COLL_WORLD(NAME)                                                                \
    template <typename T, typename Group>                                                          \
    __device__ inline int ishmemx_##NAME##_work_group(T *dest, const T *source, size_t nelems,      \
                                                      const Group &grp)                            \
    {                                                                                              \
        return ishmemx_##NAME##_work_group<T>(ISHMEMI_C_TEAM_WORLD, dest, source, nelems, grp);    \
    }                                                                                              \
    template <typename T>                                                                          \
    __device__ inline int ishmem_##NAME(int team, T *dest, const T *source, size_t nelems)         \
    {                                                                                              \
        return ishmemx_##NAME##_work_group<T>(team, dest, source, nelems, ishmemx_dev::thread);    \
    }                                                                                              \
    template <typename T>                                                                          \
    __device__ inline int ishmem_##NAME(T *dest, const T *source, size_t nelems)                   \
    {                                                                                              \
        return ishmemx_##NAME##_work_group<T>(ISHMEMI_C_TEAM_WORLD, dest, source, nelems,          \
                                              ishmemx_dev::thread);                                \
    }
ISHMEMX_DEV_COLL_WORLD(fcollect)
ISHMEMX_DEV_COLL_WORLD(collect)
ISHMEMX_DEV_COLL_WORLD(alltoall)
ISHMEMX_DEV_COLL_WORLD(sum_inscan)
ISHMEMX_DEV_COLL_WORLD(sum_exscan)
template <typename T, typename Group>
__device__ inline int ishmemx_broadcast_work_group(T *dest, const T *source, size_t nelems, int root, const Group &grp)
{
    return ishmemx_broadcast_work_group<T>(ISHMEMI_C_TEAM_WORLD, dest, source, nelems, root, grp);
}
template <typename T>
__device__ inline int ishmem_broadcast(int team, T *dest, const T *source, size_t nelems, int root)
{
    return ishmemx_broadcast_work_group<T>(team, dest, source, nelems, root, ishmemx_dev::thread);
}
template <typename T>
__device__ inline int ishmem_broadcast(T *dest, const T *source, size_t nelems, int root)
{
    return ishmemx_broadcast_work_group<T>(ISHMEMI_C_TEAM_WORLD, dest, source, nelems, root, ishmemx_dev::thread);
}

/* Typed forms for the reference's 23 arithmetic typenames (collect.cpp:44-66, :129-151,
 * scan.cpp:28-74, broadcast.cpp): work-group and one-work-item, with and without a team. */
#define ISHMEMX_DEV_COLL_TYPED_ONE(TYPENAME, TYPE, NAME)                                             \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##NAME##_work_group(int team, TYPE *dest,            \
                                                                   const TYPE *source,              \
                                                                   size_t nelems, const Group &grp) \
    {                                                                                              \
        return ishmemx_##NAME##_work_group<TYPE>(team, dest, source, nelems, grp);                 \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##NAME##_work_group(TYPE *dest, const TYPE *source,  \
                                                                   size_t nelems, const Group &grp) \
    {                                                                                              \
        return ishmemx_##NAME##_work_group<TYPE>(dest, source, nelems, grp);                       \
    }                                                                                              \
    __device__ inline int ishmem_##TYPENAME##_##NAME(int team, TYPE *dest, const TYPE *source,      \
                                                     size_t nelems)                                \
    {                                                                                              \
        return ishmem_##NAME<TYPE>(team, dest, source, nelems);                                    \
    }                                                                                              \
    __device__ inline int ishmem_##TYPENAME##_##NAME(TYPE *dest, const TYPE *source, size_t nelems) \
    {                                                                                              \
        return ishmem_##NAME<TYPE>(dest, source, nelems);                                          \
    }
#define ISHMEMX_DEV_COLL(TYPENAME, TYPE, UNUSED1, UNUSED2)                                          \
    ISHMEMX_DEV_COLL_TYPED_ONE(TYPENAME, TYPE, fcollect)                                            \
    ISHMEMX_DEV_COLL_TYPED_ONE(TYPENAME, TYPE, collect)                                             \
    ISHMEMX_DEV_COLL_TYPED_ONE(TYPENAME, TYPE, alltoall)                                            \
    ISHMEMX_DEV_COLL_TYPED_ONE(TYPENAME, TYPE, sum_inscan)                                          \
    ISHMEMX_DEV_COLL_TYPED_ONE(TYPENAME, TYPE, sum_exscan)                                          \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_broadcast_work_group(                               \
        int team, TYPE *dest, const TYPE *source, size_t nelems, int root, const Group &grp)       \
    {                                                                                              \
        return ishmemx_broadcast_work_group<TYPE>(team, dest, source, nelems, root, grp);          \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_broadcast_work_group(                               \
        TYPE *dest, const TYPE *source, size_t nelems, int root, const Group &grp)                 \
    {                                                                                              \
        return ishmemx_broadcast_work_group<TYPE>(dest, source, nelems, root, grp);                \
    }                                                                                              \
    __device__ inline int ishmem_##TYPENAME##_broadcast(int team, TYPE *dest, const TYPE *source,   \
                                                        size_t nelems, int root)                   \
    {                                                                                              \
        return ishmem_broadcast<TYPE>(team, dest, source, nelems, root);                           \
    }                                                                                              \
    __device__ inline int ishmem_##TYPENAME##_broadcast(TYPE *dest, const TYPE *source,             \
                                                        size_t nelems, int root)                   \
    {                                                                                              \
        return ishmem_broadcast<TYPE>(dest, source, nelems, root);                                 \
    }

/* byte forms: fcollectmem / collectmem / alltoallmem / broadcastmem */
template <typename Group>
__device__ inline int ishmemx_alltoallmem_work_group(int team, void *dest, const void *source, size_t nbytes,
                                                     const Group &)
{
    return ishmemx_dev::alltoall_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source, nbytes);
}
template <typename Group>
__device__ inline int ishmemx_alltoallmem_work_group(void *dest, const void *source, size_t nbytes, const Group &grp)
{
    return ishmemx_alltoallmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, grp);
}
__device__ inline int ishmem_alltoallmem(int team, void *dest, const void *source, size_t nbytes)
{
    return ishmemx_alltoallmem_work_group(team, dest, source, nbytes, ishmemx_dev::thread);
}
__device__ inline int ishmem_alltoallmem(void *dest, const void *source, size_t nbytes)
{
    return ishmemx_alltoallmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, ishmemx_dev::thread);
}
template <typename Group>
__device__ inline int ishmemx_fcollectmem_work_group(int team, void *dest, const void *source, size_t nbytes,
                                                     const Group &)
{
    return ishmemx_dev::collect_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source, nbytes,
                                                                  true);
}
template <typename Group>
__device__ inline int ishmemx_fcollectmem_work_group(void *dest, const void *source, size_t nbytes, const Group &grp)
{
    return ishmemx_fcollectmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, grp);
}
template <typename Group>
__device__ inline int ishmemx_collectmem_work_group(int team, void *dest, const void *source, size_t nbytes,
                                                    const Group &)
{
    return ishmemx_dev::collect_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source, nbytes,
                                                                  false);
}
template <typename Group>
__device__ inline int ishmemx_collectmem_work_group(void *dest, const void *source, size_t nbytes, const Group &grp)
{
    return ishmemx_collectmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, grp);
}
template <typename Group>
__device__ inline int ishmemx_broadcastmem_work_group(int team, void *dest, const void *source, size_t nbytes,
                                                      int root, const Group &)
{
    return ishmemx_dev::broadcast_group<ishmemx_dev::exec_t<Group>>(ishmemx_dev::ctx(), team, dest, source, nbytes,
                                                                    root);
}
template <typename Group>
__device__ inline int ishmemx_broadcastmem_work_group(void *dest, const void *source, size_t nbytes, int root,
                                                      const Group &grp)
{
    return ishmemx_broadcastmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, root, grp);
}
__device__ inline int ishmem_fcollectmem(int team, void *dest, const void *source, size_t nbytes)
{
    return ishmemx_fcollectmem_work_group(team, dest, source, nbytes, ishmemx_dev::thread);
}
__device__ inline int ishmem_fcollectmem(void *dest, const void *source, size_t nbytes)
{
    return ishmemx_fcollectmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, ishmemx_dev::thread);
}
__device__ inline int ishmem_collectmem(int team, void *dest, const void *source, size_t nbytes)
{
    return ishmemx_collectmem_work_group(team, dest, source, nbytes, ishmemx_dev::thread);
}
__device__ inline int ishmem_collectmem(void *dest, const void *source, size_t nbytes)
{
    return ishmemx_collectmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, ishmemx_dev::thread);
}
__device__ inline int ishmem_broadcastmem(int team, void *dest, const void *source, size_t nbytes, int root)
{
    return ishmemx_broadcastmem_work_group(team, dest, source, nbytes, root, ishmemx_dev::thread);
}
__device__ inline int ishmem_broadcastmem(void *dest, const void *source, size_t nbytes, int root)
{
    return ishmemx_broadcastmem_work_group(ISHMEMI_C_TEAM_WORLD, dest, source, nbytes, root, ishmemx_dev::thread);
}

/* Same TYPENAME x op matrix as the host API (src/collectives/reduce.cpp:95-417). */
#define ISHMEMX_DEV_BITWISE_TYPES(X, OPNAME, OPC)                                                   \
    X(uchar, unsigned char, OPNAME, OPC) X(ushort, unsigned short, OPNAME, OPC)                    \
    X(uint, unsigned int, OPNAME, OPC) X(ulong, unsigned long, OPNAME, OPC)                        \
    X(ulonglong, unsigned long long, OPNAME, OPC) X(int8, int8_t, OPNAME, OPC)                     \
    X(int16, int16_t, OPNAME, OPC) X(int32, int32_t, OPNAME, OPC) X(int64, int64_t, OPNAME, OPC)   \
    X(uint8, uint8_t, OPNAME, OPC) X(uint16, uint16_t, OPNAME, OPC)                                \
    X(uint32, uint32_t, OPNAME, OPC) X(uint64, uint64_t, OPNAME, OPC) X(size, size_t, OPNAME, OPC)
#define ISHMEMX_DEV_ARITH_TYPES(X, OPNAME, OPC)                                                     \
    X(char, char, OPNAME, OPC) X(schar, signed char, OPNAME, OPC) X(short, short, OPNAME, OPC)     \
    X(int, int, OPNAME, OPC) X(long, long, OPNAME, OPC) X(longlong, long long, OPNAME, OPC)        \
    X(ptrdiff, ptrdiff_t, OPNAME, OPC) X(uchar, unsigned char, OPNAME, OPC)                        \
    X(ushort, unsigned short, OPNAME, OPC) X(uint, unsigned int, OPNAME, OPC)                      \
    X(ulong, unsigned long, OPNAME, OPC) X(ulonglong, unsigned long long, OPNAME, OPC)             \
    X(int8, int8_t, OPNAME, OPC) X(int16, int16_t, OPNAME, OPC) X(int32, int32_t, OPNAME, OPC)     \
    X(int64, int64_t, OPNAME, OPC) X(uint8, uint8_t, OPNAME, OPC) X(uint16, uint16_t, OPNAME, OPC) \
    X(uint32, uint32_t, OPNAME, OPC) X(uint64, uint64_t, OPNAME, OPC) X(size, size_t, OPNAME, OPC) \
    X(float, float, OPNAME, OPC) X(double, double, OPNAME, OPC)

ISHMEMX_DEV_BITWISE_TYPES(ISHMEMX_DEV_TYPED, and, ISHMEMI_OP_AND)
ISHMEMX_DEV_BITWISE_TYPES(ISHMEMX_DEV_TYPED, or, ISHMEMI_OP_OR)
ISHMEMX_DEV_BITWISE_TYPES(ISHMEMX_DEV_TYPED, xor, ISHMEMI_OP_XOR)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_TYPED, max, ISHMEMI_OP_MAX)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_TYPED, min, ISHMEMI_OP_MIN)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_TYPED, sum, ISHMEMI_OP_SUM)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_TYPED, prod, ISHMEMI_OP_PROD)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_COLL, _, _)

/* Extension (no reference counterpart): the 16-bit floating-point reductions from a kernel,
 *   ishmemx_{half,bfloat16}_{max,min,sum,prod}_reduce_work_group([team,] dest, source, nreduce, grp)
 *   ishmemx_{half,bfloat16}_{max,min,sum,prod}_reduce([team,] dest, source, nreduce)   (one work-item)
 * on ishmemx_half_t / ishmemx_bfloat16_t; the generic forms above also take _Float16, __half,
 * __bf16 and __hip_bfloat16.  Same team-order, round-every-step fold as the host path. */
#define ISHMEMX_DEV_FP16_TYPED(TYPENAME, TYPE, OPNAME, OPC)                                         \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_work_group(                       \
        TYPE *dest, const TYPE *source, size_t nreduce, const Group &grp)                          \
    {                                                                                              \
        return ishmemx_##OPNAME##_reduce_work_group<TYPE>(dest, source, nreduce, grp);             \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_work_group(                       \
        int team, TYPE *dest, const TYPE *source, size_t nreduce, const Group &grp)                \
    {                                                                                              \
        return ishmemx_##OPNAME##_reduce_work_group<TYPE>(team, dest, source, nreduce, grp);       \
    }                                                                                              \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce(TYPE *dest, const TYPE *source,   \
                                                                 size_t nreduce)                   \
    {                                                                                              \
        return ishmem_##OPNAME##_reduce<TYPE>(dest, source, nreduce);                              \
    }                                                                                              \
    __device__ inline int ishmemx_##TYPENAME##_##OPNAME##_reduce(int team, TYPE *dest,             \
                                                                 const TYPE *source, size_t nreduce) \
    {                                                                                              \
        return ishmem_##OPNAME##_reduce<TYPE>(team, dest, source, nreduce);                        \
    }
#define ISHMEMX_DEV_FP16_TYPES(X, OPNAME, OPC)                                                      \
    X(half, ishmemx_half_t, OPNAME, OPC) X(bfloat16, ishmemx_bfloat16_t, OPNAME, OPC)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_FP16_TYPED, max, ISHMEMI_OP_MAX)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_FP16_TYPED, min, ISHMEMI_OP_MIN)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_FP16_TYPED, sum, ISHMEMI_OP_SUM)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_FP16_TYPED, prod, ISHMEMI_OP_PROD)

/* The reduce-scatter extension's typed names: the reduce's matrix and the two 16-bit types. */
ISHMEMX_DEV_BITWISE_TYPES(ISHMEMX_DEV_RS_TYPED, and, ISHMEMI_OP_AND)
ISHMEMX_DEV_BITWISE_TYPES(ISHMEMX_DEV_RS_TYPED, or, ISHMEMI_OP_OR)
ISHMEMX_DEV_BITWISE_TYPES(ISHMEMX_DEV_RS_TYPED, xor, ISHMEMI_OP_XOR)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_RS_TYPED, max, ISHMEMI_OP_MAX)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_RS_TYPED, min, ISHMEMI_OP_MIN)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_RS_TYPED, sum, ISHMEMI_OP_SUM)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_RS_TYPED, prod, ISHMEMI_OP_PROD)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_RS_TYPED, max, ISHMEMI_OP_MAX)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_RS_TYPED, min, ISHMEMI_OP_MIN)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_RS_TYPED, sum, ISHMEMI_OP_SUM)
ISHMEMX_DEV_FP16_TYPES(ISHMEMX_DEV_RS_TYPED, prod, ISHMEMI_OP_PROD)

/* ---- put / get / p / g, quiet / fence from a kernel (src/ishmem.h:90-330, src/ishmemx.h) --------
 * ishmem_<TN>_put / _get (one work-item; every calling work-item moves its own arguments),
 * ishmemx_<TN>_put_work_group / _get_work_group (every thread of the group, same arguments), their
 * _nbi forms (complete eagerly here), sized (8..128) and mem forms, ishmem_<TN>_p / _g (one
 * system-scope store / load: g is never served from a warm cache line), ishmem_quiet / fence and
 * ishmemx_quiet_work_group / fence_work_group.  dest of a put / source of a get: symmetric-heap
 * address.  Visibility on the target: DESIGN.md §3b. */
#define ISHMEMX_DEV_RMA_GENERIC(NAME, PUT)                                                          \
    template <typename T>                                                                          \
    __device__ inline void ishmem_##NAME(T *dest, const T *source, size_t nelems, int pe)          \
    {                                                                                              \
        ishmemx_dev::rma_call<ishmemx_dev::thread_t, PUT>((void *) dest, (const void *) source, nelems * sizeof(T), pe); \
    }                                                                                              \
    template <typename T, typename Group>                                                          \
    __device__ inline void ishmemx_##NAME##_work_group(T *dest, const T *source, size_t nelems, int pe, const Group &) \
    {                                                                                              \
        ishmemx_dev::rma_call<ishmemx_dev::exec_t<Group>, PUT>((void *) dest, (const void *) source, \
                                                               nelems * sizeof(T), pe);            \
    }
ISHMEMX_DEV_RMA_GENERIC(put, true)
ISHMEMX_DEV_RMA_GENERIC(get, false)
ISHMEMX_DEV_RMA_GENERIC(put_nbi, true)
ISHMEMX_DEV_RMA_GENERIC(get_nbi, false)
#define ISHMEMX_DEV_RMA_MEM(NAME, PUT, MUL)                                                         \
    __device__ inline void ishmem_##NAME(void *dest, const void *source, size_t n, int pe)         \
    {                                                                                              \
        ishmemx_dev::rma_call<ishmemx_dev::thread_t, PUT>(dest, source, n * (MUL), pe);            \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_##NAME##_work_group(void *dest, const void *source, size_t n, int pe, const Group &) \
    {                                                                                              \
        ishmemx_dev::rma_call<ishmemx_dev::exec_t<Group>, PUT>(dest, source, n * (MUL), pe);       \
    }
#define ISHMEMX_DEV_RMA_MEM_BOTH(SUFFIX, MUL)                                                       \
    ISHMEMX_DEV_RMA_MEM(put##SUFFIX, true, MUL)                                                     \
    ISHMEMX_DEV_RMA_MEM(get##SUFFIX, false, MUL)                                                    \
    ISHMEMX_DEV_RMA_MEM(put##SUFFIX##_nbi, true, MUL)                                               \
    ISHMEMX_DEV_RMA_MEM(get##SUFFIX##_nbi, false, MUL)
ISHMEMX_DEV_RMA_MEM_BOTH(mem, 1)
ISHMEMX_DEV_RMA_MEM_BOTH(8, 1)
ISHMEMX_DEV_RMA_MEM_BOTH(16, 2)
ISHMEMX_DEV_RMA_MEM_BOTH(32, 4)
ISHMEMX_DEV_RMA_MEM_BOTH(64, 8)
ISHMEMX_DEV_RMA_MEM_BOTH(128, 16)
template <typename T>
__device__ inline void ishmem_p(T *dest, T value, int pe)
{
    static_assert(sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8, "ishmem_p: 1, 2, 4 or 8 bytes");
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    if (!c || pe < 0 || pe >= c->npes) return;
    ishmemx_dev::sys_store((T *) ishmemx_dev::peer_addr(c, dest, pe), value);
}
template <typename T>
__device__ inline T ishmem_g(const T *source, int pe)
{
    static_assert(sizeof(T) == 1 || sizeof(T) == 2 || sizeof(T) == 4 || sizeof(T) == 8, "ishmem_g: 1, 2, 4 or 8 bytes");
    const ishmemi_c_device_ctx_t *c = ishmemx_dev::ctx();
    if (!c || pe < 0 || pe >= c->npes) return T();
    return ishmemx_dev::sys_load((const T *) ishmemx_dev::peer_addr(c, source, pe));
}
#define ISHMEMX_DEV_RMA_TYPED_ONE(TYPENAME, TYPE, NAME)                                             \
    __device__ inline void ishmem_##TYPENAME##_##NAME(TYPE *d, const TYPE *s, size_t n, int pe)    \
    {                                                                                              \
        ishmem_##NAME<TYPE>(d, s, n, pe);                                                          \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_##TYPENAME##_##NAME##_work_group(TYPE *d, const TYPE *s, size_t n, int pe, \
                                                                    const Group &grp)              \
    {                                                                                              \
        ishmemx_##NAME##_work_group<TYPE>(d, s, n, pe, grp);                                       \
    }
#define ISHMEMX_DEV_RMA_TYPED(TYPENAME, TYPE, UNUSED1, UNUSED2)                                     \
    ISHMEMX_DEV_RMA_TYPED_ONE(TYPENAME, TYPE, put)                                                  \
    ISHMEMX_DEV_RMA_TYPED_ONE(TYPENAME, TYPE, get)                                                  \
    ISHMEMX_DEV_RMA_TYPED_ONE(TYPENAME, TYPE, put_nbi)                                              \
    ISHMEMX_DEV_RMA_TYPED_ONE(TYPENAME, TYPE, get_nbi)                                              \
    __device__ inline void ishmem_##TYPENAME##_p(TYPE *d, TYPE v, int pe) { ishmem_p<TYPE>(d, v, pe); } \
    __device__ inline TYPE ishmem_##TYPENAME##_g(const TYPE *s, int pe) { return ishmem_g<TYPE>(s, pe); }
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_RMA_TYPED, _, _)
/* Strided / blocked put / get from a kernel (src/ishmem.h:122-150, :211-239, src/ishmemx.h:137-480):
 * ishmem_<TN>_iput / _iget and ishmemx_<TN>_ibput / _ibget (one work-item, its own arguments),
 * ishmemx_<TN>_iput_work_group / _iget_work_group / _ibput_work_group / _ibget_work_group (every thread
 * of the group, same arguments), the generic templates and the sized forms (8..128; the 128-bit forms
 * count 16-byte elements and strides).  Element strides, >= 1 and >= bsize. */
#define ISHMEMX_DEV_STRIDED_GENERIC(DIR, PUT)                                                       \
    template <typename T>                                                                          \
    __device__ inline void ishmem_i##DIR(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, size_t nelems, int pe) \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::thread_t, PUT>((void *) dest, (const void *) source, dst, sst, 1, \
                                                                  nelems, sizeof(T), pe);          \
    }                                                                                              \
    template <typename T, typename Group>                                                          \
    __device__ inline void ishmemx_i##DIR##_work_group(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, \
                                                       size_t nelems, int pe, const Group &)       \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::exec_t<Group>, PUT>((void *) dest, (const void *) source, dst, sst, \
                                                                       1, nelems, sizeof(T), pe);  \
    }                                                                                              \
    template <typename T>                                                                          \
    __device__ inline void ishmemx_ib##DIR(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                           size_t nblocks, int pe)                                 \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::thread_t, PUT>((void *) dest, (const void *) source, dst, sst, \
                                                                  bsize, nblocks, sizeof(T), pe);  \
    }                                                                                              \
    template <typename T, typename Group>                                                          \
    __device__ inline void ishmemx_ib##DIR##_work_group(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, \
                                                        size_t bsize, size_t nblocks, int pe, const Group &) \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::exec_t<Group>, PUT>((void *) dest, (const void *) source, dst, sst, \
                                                                       bsize, nblocks, sizeof(T), pe); \
    }
ISHMEMX_DEV_STRIDED_GENERIC(put, true)
ISHMEMX_DEV_STRIDED_GENERIC(get, false)
#define ISHMEMX_DEV_STRIDED_SIZED(DIR, PUT, BITS)                                                   \
    __device__ inline void ishmem_i##DIR##BITS(void *dest, const void *source, ptrdiff_t dst, ptrdiff_t sst, size_t n, \
                                               int pe)                                             \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::thread_t, PUT>(dest, source, dst, sst, 1, n, BITS / 8, pe); \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_i##DIR##BITS##_work_group(void *dest, const void *source, ptrdiff_t dst, \
                                                             ptrdiff_t sst, size_t n, int pe, const Group &) \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::exec_t<Group>, PUT>(dest, source, dst, sst, 1, n, BITS / 8, pe); \
    }                                                                                              \
    __device__ inline void ishmemx_ib##DIR##BITS(void *dest, const void *source, ptrdiff_t dst, ptrdiff_t sst, \
                                                 size_t bsize, size_t nblocks, int pe)             \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::thread_t, PUT>(dest, source, dst, sst, bsize, nblocks, BITS / 8, pe); \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_ib##DIR##BITS##_work_group(void *dest, const void *source, ptrdiff_t dst, \
                                                              ptrdiff_t sst, size_t bsize, size_t nblocks, int pe, \
                                                              const Group &)                       \
    {                                                                                              \
        ishmemx_dev::rma_strided_call<ishmemx_dev::exec_t<Group>, PUT>(dest, source, dst, sst, bsize, nblocks, \
                                                                       BITS / 8, pe);              \
    }
#define ISHMEMX_DEV_STRIDED_SIZED_BOTH(BITS)                                                        \
    ISHMEMX_DEV_STRIDED_SIZED(put, true, BITS)                                                      \
    ISHMEMX_DEV_STRIDED_SIZED(get, false, BITS)
ISHMEMX_DEV_STRIDED_SIZED_BOTH(8)
ISHMEMX_DEV_STRIDED_SIZED_BOTH(16)
ISHMEMX_DEV_STRIDED_SIZED_BOTH(32)
ISHMEMX_DEV_STRIDED_SIZED_BOTH(64)
ISHMEMX_DEV_STRIDED_SIZED_BOTH(128)
#define ISHMEMX_DEV_STRIDED_TYPED_ONE(TYPENAME, TYPE, DIR)                                          \
    __device__ inline void ishmem_##TYPENAME##_i##DIR(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, \
                                                      int pe)                                      \
    {                                                                                              \
        ishmem_i##DIR<TYPE>(d, s, dst, sst, n, pe);                                                \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_##TYPENAME##_i##DIR##_work_group(TYPE *d, const TYPE *s, ptrdiff_t dst, \
                                                                    ptrdiff_t sst, size_t n, int pe, const Group &grp) \
    {                                                                                              \
        ishmemx_i##DIR##_work_group<TYPE>(d, s, dst, sst, n, pe, grp);                             \
    }                                                                                              \
    __device__ inline void ishmemx_##TYPENAME##_ib##DIR(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, \
                                                        size_t bsize, size_t nblocks, int pe)      \
    {                                                                                              \
        ishmemx_ib##DIR<TYPE>(d, s, dst, sst, bsize, nblocks, pe);                                 \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_##TYPENAME##_ib##DIR##_work_group(TYPE *d, const TYPE *s, ptrdiff_t dst, \
                                                                     ptrdiff_t sst, size_t bsize, size_t nblocks, \
                                                                     int pe, const Group &grp)     \
    {                                                                                              \
        ishmemx_ib##DIR##_work_group<TYPE>(d, s, dst, sst, bsize, nblocks, pe, grp);               \
    }
#define ISHMEMX_DEV_STRIDED_TYPED(TYPENAME, TYPE, UNUSED1, UNUSED2)                                 \
    ISHMEMX_DEV_STRIDED_TYPED_ONE(TYPENAME, TYPE, put)                                              \
    ISHMEMX_DEV_STRIDED_TYPED_ONE(TYPENAME, TYPE, get)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_STRIDED_TYPED, _, _)
__device__ inline void ishmem_quiet(void) { ishmemx_dev::quiet_group<ishmemx_dev::thread_t>(); }
__device__ inline void ishmem_fence(void) { ishmemx_dev::quiet_group<ishmemx_dev::thread_t>(); }
template <typename Group>
__device__ inline void ishmemx_quiet_work_group(const Group &)
{
    ishmemx_dev::quiet_group<ishmemx_dev::exec_t<Group>>();
}
template <typename Group>
__device__ inline void ishmemx_fence_work_group(const Group &)
{
    ishmemx_dev::quiet_group<ishmemx_dev::exec_t<Group>>();
}

/* ---- put with signal, signal operations, wait_until / test from a kernel (src/ishmem.h:640-705,
 *      :1320-1354, :1551-1552, src/ishmemx.h:608-738, :1906-1920, :2011-2040, :2221-2226) ------------
 * ishmem_<TN>_put_signal[_nbi] (one work-item), ishmemx_<TN>_put_signal[_nbi]_work_group (a thread
 * block or a 64-lane tile, same arguments in every thread), sized and mem forms; ishmemx_signal_set /
 * _add; ishmem_signal_fetch; ishmem_signal_wait_until, ishmem_<TN>_wait_until / _test and their
 * _work_group forms for the 12 synchronisation typenames.  After a wait (or a test that returned 1)
 * plain loads of the bytes the signal announced see them.  Every wait is bounded by the library's
 * timeout; a timed-out wait returns (signal_wait_until: the last value read) and shows in
 * ishmemi_c_error_count().  DESIGN.md §3c. */
#define ISHMEMX_DEV_PUT_SIGNAL_GENERIC(NAME)                                                        \
    template <typename T>                                                                          \
    __device__ inline void ishmem_##NAME(T *dest, const T *source, size_t nelems, uint64_t *sig_addr, uint64_t signal, \
                                         int sig_op, int pe)                                       \
    {                                                                                              \
        ishmemx_dev::put_signal_call<ishmemx_dev::thread_t>((void *) dest, (const void *) source, nelems * sizeof(T), \
                                                            sig_addr, signal, sig_op, pe);         \
    }                                                                                              \
    template <typename T, typename Group>                                                          \
    __device__ inline void ishmemx_##NAME##_work_group(T *dest, const T *source, size_t nelems, uint64_t *sig_addr,    \
                                                       uint64_t signal, int sig_op, int pe, const Group &)       \
    {                                                                                              \
        ishmemx_dev::put_signal_call<ishmemx_dev::exec_t<Group>>((void *) dest, (const void *) source,           \
                                                                 nelems * sizeof(T), sig_addr, signal, sig_op, pe); \
    }
ISHMEMX_DEV_PUT_SIGNAL_GENERIC(put_signal)
ISHMEMX_DEV_PUT_SIGNAL_GENERIC(put_signal_nbi)
#define ISHMEMX_DEV_PUT_SIGNAL_MEM(NAME, MUL)                                                       \
    __device__ inline void ishmem_##NAME(void *dest, const void *source, size_t n, uint64_t *sig_addr, uint64_t signal, \
                                         int sig_op, int pe)                                       \
    {                                                                                              \
        ishmemx_dev::put_signal_call<ishmemx_dev::thread_t>(dest, source, n * (MUL), sig_addr, signal, sig_op, pe); \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_##NAME##_work_group(void *dest, const void *source, size_t n, uint64_t *sig_addr,   \
                                                       uint64_t signal, int sig_op, int pe, const Group &)       \
    {                                                                                              \
        ishmemx_dev::put_signal_call<ishmemx_dev::exec_t<Group>>(dest, source, n * (MUL), sig_addr, signal, sig_op, pe); \
    }
#define ISHMEMX_DEV_PUT_SIGNAL_MEM_BOTH(SUFFIX, MUL)                                                \
    ISHMEMX_DEV_PUT_SIGNAL_MEM(put##SUFFIX##_signal, MUL)                                           \
    ISHMEMX_DEV_PUT_SIGNAL_MEM(put##SUFFIX##_signal_nbi, MUL)
ISHMEMX_DEV_PUT_SIGNAL_MEM_BOTH(mem, 1)
ISHMEMX_DEV_PUT_SIGNAL_MEM_BOTH(8, 1)
ISHMEMX_DEV_PUT_SIGNAL_MEM_BOTH(16, 2)
ISHMEMX_DEV_PUT_SIGNAL_MEM_BOTH(32, 4)
ISHMEMX_DEV_PUT_SIGNAL_MEM_BOTH(64, 8)
ISHMEMX_DEV_PUT_SIGNAL_MEM_BOTH(128, 16)
#define ISHMEMX_DEV_PUT_SIGNAL_TYPED_ONE(TYPENAME, TYPE, NAME)                                      \
    __device__ inline void ishmem_##TYPENAME##_##NAME(TYPE *d, const TYPE *s, size_t n, uint64_t *sig, uint64_t v,     \
                                                      int op, int pe)                              \
    {                                                                                              \
        ishmem_##NAME<TYPE>(d, s, n, sig, v, op, pe);                                              \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_##TYPENAME##_##NAME##_work_group(TYPE *d, const TYPE *s, size_t n, uint64_t *sig,   \
                                                                    uint64_t v, int op, int pe, const Group &grp) \
    {                                                                                              \
        ishmemx_##NAME##_work_group<TYPE>(d, s, n, sig, v, op, pe, grp);                           \
    }
#define ISHMEMX_DEV_PUT_SIGNAL_TYPED(TYPENAME, TYPE, UNUSED1, UNUSED2)                              \
    ISHMEMX_DEV_PUT_SIGNAL_TYPED_ONE(TYPENAME, TYPE, put_signal)                                    \
    ISHMEMX_DEV_PUT_SIGNAL_TYPED_ONE(TYPENAME, TYPE, put_signal_nbi)
ISHMEMX_DEV_ARITH_TYPES(ISHMEMX_DEV_PUT_SIGNAL_TYPED, _, _)

__device__ inline void ishmemx_signal_set(uint64_t *sig_addr, uint64_t signal, int pe)
{
    ishmemx_dev::signal_op_call(sig_addr, signal, ISHMEMI_C_SIGNAL_SET, pe);
}
__device__ inline void ishmemx_signal_add(uint64_t *sig_addr, uint64_t signal, int pe)
{
    ishmemx_dev::signal_op_call(sig_addr, signal, ISHMEMI_C_SIGNAL_ADD, pe);
}
__device__ inline uint64_t ishmem_signal_fetch(uint64_t *sig_addr) { return ishmemx_dev::sys_load(sig_addr); }
__device__ inline uint64_t ishmem_signal_wait_until(uint64_t *sig_addr, int cmp, uint64_t cmp_value)
{
    return ishmemx_dev::wait_until_group<ishmemx_dev::thread_t, uint64_t>(sig_addr, cmp, cmp_value, 0, nullptr);
}
template <typename Group>
__device__ inline uint64_t ishmemx_signal_wait_until_work_group(uint64_t *sig_addr, int cmp, uint64_t cmp_value,
                                                                const Group &)
{
    return ishmemx_dev::wait_until_group<ishmemx_dev::exec_t<Group>, uint64_t>(sig_addr, cmp, cmp_value, 0, nullptr);
}
template <typename T>
__device__ inline void ishmem_wait_until(T *ivar, int cmp, T cmp_value)
{
    (void) ishmemx_dev::wait_until_group<ishmemx_dev::thread_t, T>(ivar, cmp, cmp_value, 0, nullptr);
}
template <typename T>
__device__ inline int ishmem_test(T *ivar, int cmp, T cmp_value)
{
    int m = 0;
    (void) ishmemx_dev::wait_until_group<ishmemx_dev::thread_t, T>(ivar, cmp, cmp_value, 1, &m);
    return m;
}
template <typename T, typename Group>
__device__ inline void ishmemx_wait_until_work_group(T *ivar, int cmp, T cmp_value, const Group &)
{
    (void) ishmemx_dev::wait_until_group<ishmemx_dev::exec_t<Group>, T>(ivar, cmp, cmp_value, 0, nullptr);
}
template <typename T, typename Group>
__device__ inline int ishmemx_test_work_group(T *ivar, int cmp, T cmp_value, const Group &)
{
    int m = 0;
    (void) ishmemx_dev::wait_until_group<ishmemx_dev::exec_t<Group>, T>(ivar, cmp, cmp_value, 1, &m);
    return m;
}
#define ISHMEMX_DEV_SYNC_TYPES(X)                                                                   \
    X(int, int) X(long, long) X(longlong, long long) X(uint, unsigned int) X(ulong, unsigned long)  \
    X(ulonglong, unsigned long long) X(int32, int32_t) X(int64, int64_t) X(uint32, uint32_t)        \
    X(uint64, uint64_t) X(size, size_t) X(ptrdiff, ptrdiff_t)
#define ISHMEMX_DEV_SYNC_TYPED(TYPENAME, TYPE)                                                      \
    __device__ inline void ishmem_##TYPENAME##_wait_until(TYPE *ivar, int cmp, TYPE v) { ishmem_wait_until<TYPE>(ivar, cmp, v); } \
    __device__ inline int ishmem_##TYPENAME##_test(TYPE *ivar, int cmp, TYPE v) { return ishmem_test<TYPE>(ivar, cmp, v); } \
    template <typename Group>                                                                      \
    __device__ inline void ishmemx_##TYPENAME##_wait_until_work_group(TYPE *ivar, int cmp, TYPE v, const Group &grp)   \
    {                                                                                              \
        ishmemx_wait_until_work_group<TYPE>(ivar, cmp, v, grp);                                    \
    }                                                                                              \
    template <typename Group>                                                                      \
    __device__ inline int ishmemx_##TYPENAME##_test_work_group(TYPE *ivar, int cmp, TYPE v, const Group &grp)          \
    {                                                                                              \
        return ishmemx_test_work_group<TYPE>(ivar, cmp, v, grp);                                   \
    }
ISHMEMX_DEV_SYNC_TYPES(ISHMEMX_DEV_SYNC_TYPED)

/* ---- vector waits and tests from a kernel (src/ishmem.h:1343-1538, src/ishmemx.h:1908-2208) --------
 * ishmem_<TN>_wait_until_all / _any / _some[_vector] and ishmem_<TN>_test_all / _any / _some[_vector],
 * callable by one work-item (divergent callers are legal), the templates, and their
 * ishmemx_..._work_group forms for a thread block, a 64-lane tile and the library's tags (same
 * arguments in every thread; every thread gets the result, and after a some form every thread may
 * read indices[0 .. count)).  When a call reports a match, plain loads of the data the variables
 * announce see it, in every thread of the group.  Waits are bounded by the library's timeout: a
 * timed-out wait returns (any: SIZE_MAX, some: 0) and shows in ishmemi_c_error_count().  An invalid
 * cmp or a missing array returns at once and is recorded too.  DESIGN.md §3f. */
ISHMEMI_SYNC_VECTOR_GENERIC(__device__ inline, ishmemx_dev)
#define ISHMEMX_DEV_SYNC_VECTOR_TYPED(TYPENAME, TYPE)                                               \
    ISHMEMI_SYNC_VECTOR_TYPED_FORM(__device__ inline, TYPENAME, TYPE, , TYPE v)                     \
    ISHMEMI_SYNC_VECTOR_TYPED_FORM(__device__ inline, TYPENAME, TYPE, _vector, const TYPE *v)
ISHMEMX_DEV_SYNC_TYPES(ISHMEMX_DEV_SYNC_VECTOR_TYPED)
/* The six group operations of one form, named PREFIX<op>SUFFIX; CV and the trailing arguments:
 * `T v` and `v, nullptr` (scalar), `const T *v` and `T(), v` (_vector). */
#define ISHMEMX_DEV_SYNC_VECTOR_WG_FORM(TEMPLATE, PREFIX, SUFFIX, T, MODEBITS, CV, ...)             \
    TEMPLATE __device__ inline void PREFIX##wait_until_all##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV, \
                                                                   const Group &)                  \
    {                                                                                              \
        (void) ishmemx_dev::sync_vector_group<ishmemx_dev::exec_t<Group>, T>(ISHMEMI_C_SYNC_WAIT_ALL | MODEBITS, ivars, n, \
                                                                             nullptr, status, cmp, __VA_ARGS__); \
    }                                                                                              \
    TEMPLATE __device__ inline size_t PREFIX##wait_until_any##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV, \
                                                                     const Group &)                \
    {                                                                                              \
        return ishmemx_dev::sync_vector_group<ishmemx_dev::exec_t<Group>, T>(ISHMEMI_C_SYNC_WAIT_ANY | MODEBITS, ivars, n, \
                                                                             nullptr, status, cmp, __VA_ARGS__); \
    }                                                                                              \
    TEMPLATE __device__ inline size_t PREFIX##wait_until_some##SUFFIX(T *ivars, size_t n, size_t *indices, const int *status, \
                                                                      int cmp, CV, const Group &)  \
    {                                                                                              \
        return ishmemx_dev::sync_vector_group<ishmemx_dev::exec_t<Group>, T>(ISHMEMI_C_SYNC_WAIT_SOME | MODEBITS, ivars, n, \
                                                                             indices, status, cmp, __VA_ARGS__); \
    }                                                                                              \
    TEMPLATE __device__ inline int PREFIX##test_all##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV, const Group &) \
    {                                                                                              \
        return (int) ishmemx_dev::sync_vector_group<ishmemx_dev::exec_t<Group>, T>(ISHMEMI_C_SYNC_TEST_ALL | MODEBITS, ivars, \
                                                                                   n, nullptr, status, cmp, __VA_ARGS__); \
    }                                                                                              \
    TEMPLATE __device__ inline size_t PREFIX##test_any##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV,   \
                                                               const Group &)                      \
    {                                                                                              \
        return ishmemx_dev::sync_vector_group<ishmemx_dev::exec_t<Group>, T>(ISHMEMI_C_SYNC_TEST_ANY | MODEBITS, ivars, n, \
                                                                             nullptr, status, cmp, __VA_ARGS__); \
    }                                                                                              \
    TEMPLATE __device__ inline size_t PREFIX##test_some##SUFFIX(T *ivars, size_t n, size_t *indices, const int *status, \
                                                                int cmp, CV, const Group &)        \
    {                                                                                              \
        return ishmemx_dev::sync_vector_group<ishmemx_dev::exec_t<Group>, T>(ISHMEMI_C_SYNC_TEST_SOME | MODEBITS, ivars, n, \
                                                                             indices, status, cmp, __VA_ARGS__); \
    }
#define ISHMEMX_DEV_TEMPLATE_T_GROUP template <typename T, typename Group>
#define ISHMEMX_DEV_TEMPLATE_GROUP template <typename Group>
ISHMEMX_DEV_SYNC_VECTOR_WG_FORM(ISHMEMX_DEV_TEMPLATE_T_GROUP, ishmemx_, _work_group, T, 0, T v, v, (const T *) nullptr)
ISHMEMX_DEV_SYNC_VECTOR_WG_FORM(ISHMEMX_DEV_TEMPLATE_T_GROUP, ishmemx_, _vector_work_group, T, ISHMEMI_C_SYNC_VECTOR,
                                const T *v, T(), v)
#define ISHMEMX_DEV_SYNC_VECTOR_WG_TYPED(TYPENAME, TYPE)                                            \
    ISHMEMX_DEV_SYNC_VECTOR_WG_FORM(ISHMEMX_DEV_TEMPLATE_GROUP, ishmemx_##TYPENAME##_, _work_group, TYPE, 0, TYPE v, v, \
                                    (const TYPE *) nullptr)                                        \
    ISHMEMX_DEV_SYNC_VECTOR_WG_FORM(ISHMEMX_DEV_TEMPLATE_GROUP, ishmemx_##TYPENAME##_, _vector_work_group, TYPE,     \
                                    ISHMEMI_C_SYNC_VECTOR, const TYPE *v, (TYPE) 0, v)
ISHMEMX_DEV_SYNC_TYPES(ISHMEMX_DEV_SYNC_VECTOR_WG_TYPED)

/* ---- atomic memory operations from a kernel (src/ishmem.h:331-640) -----------------
 * ishmem_atomic_<op>[_nbi]<T> and ishmem_<TYPENAME>_atomic_<op>[_nbi] (ishmem_amo.h), callable by one
 * work-item; every lane of a wave may call, with the same or with different dest / pe.  One relaxed
 * system-scope builtin on the word's bits at the peer-mapped address: no compare-and-swap loop, the
 * vector path.  A fetching form returns the old value; an _nbi form stores it to *fetch, valid after
 * the calling work-item's ishmem_quiet(); a non-fetching form is a no-return atomic, complete after
 * ishmem_quiet() / ishmem_fence() (their s_waitcnt vmcnt(0) counts it).  AMOs order nothing else by
 * themselves.  A pe outside [0, npes) returns at once, a fetching form T(). */
namespace ishmemx_dev {
template <typename U>
__device__ __forceinline__ U amo_rmw(int op, U *p, U v, U cond)
{
    constexpr int kOrder = __ATOMIC_RELAXED, kScope = __HIP_MEMORY_SCOPE_SYSTEM;
    switch (op) {
        case ISHMEMI_C_AMO_FETCH: return __hip_atomic_load(p, kOrder, kScope);
        case ISHMEMI_C_AMO_SWAP: return __hip_atomic_exchange(p, v, kOrder, kScope);
        case ISHMEMI_C_AMO_COMPARE_SWAP:
            (void) __hip_atomic_compare_exchange_strong(p, &cond, v, kOrder, kOrder, kScope);
            return cond;  // the word's value before the operation, whether it matched or not
        case ISHMEMI_C_AMO_FETCH_INC: return __hip_atomic_fetch_add(p, (U) 1, kOrder, kScope);
        case ISHMEMI_C_AMO_FETCH_ADD: return __hip_atomic_fetch_add(p, v, kOrder, kScope);
        case ISHMEMI_C_AMO_FETCH_AND: return __hip_atomic_fetch_and(p, v, kOrder, kScope);
        case ISHMEMI_C_AMO_FETCH_OR: return __hip_atomic_fetch_or(p, v, kOrder, kScope);
        default: return __hip_atomic_fetch_xor(p, v, kOrder, kScope);
    }
}
template <typename T>
__device__ __forceinline__ T amo_f(int op, T *dest, T val, T cond, int pe)
{
    using U = ishmemi_amo::bits_t<T>;
    const ishmemi_c_device_ctx_t *c = ctx();
    if (!c || pe < 0 || pe >= c->npes) return T();
    const U old = amo_rmw<U>(op, (U *) peer_addr(c, dest, pe), __builtin_bit_cast(U, val), __builtin_bit_cast(U, cond));
    return __builtin_bit_cast(T, old);
}
template <typename T>
__device__ __forceinline__ void amo_v(int op, T *dest, T val, int pe)
{
    using U = ishmemi_amo::bits_t<T>;
    constexpr int kOrder = __ATOMIC_RELAXED, kScope = __HIP_MEMORY_SCOPE_SYSTEM;
    const ishmemi_c_device_ctx_t *c = ctx();
    if (!c || pe < 0 || pe >= c->npes) return;
    U *p = (U *) peer_addr(c, dest, pe);
    const U v = __builtin_bit_cast(U, val);
    switch (op) {
        case ISHMEMI_C_AMO_SET: __hip_atomic_store(p, v, kOrder, kScope); break;
        case ISHMEMI_C_AMO_INC: (void) __hip_atomic_fetch_add(p, (U) 1, kOrder, kScope); break;
        case ISHMEMI_C_AMO_ADD: (void) __hip_atomic_fetch_add(p, v, kOrder, kScope); break;
        case ISHMEMI_C_AMO_AND: (void) __hip_atomic_fetch_and(p, v, kOrder, kScope); break;
        case ISHMEMI_C_AMO_OR: (void) __hip_atomic_fetch_or(p, v, kOrder, kScope); break;
        default: (void) __hip_atomic_fetch_xor(p, v, kOrder, kScope); break;
    }
}
template <typename T>
__device__ __forceinline__ void amo_n(int op, T *fetch, T *dest, T val, T cond, int pe)
{
    using U = ishmemi_amo::bits_t<T>;
    const ishmemi_c_device_ctx_t *c = ctx();
    if (!c || pe < 0 || pe >= c->npes) return;
    const U old = amo_rmw<U>(op, (U *) peer_addr(c, dest, pe), __builtin_bit_cast(U, val), __builtin_bit_cast(U, cond));
    *(U *) fetch = old;
}
}  // namespace ishmemx_dev
ISHMEMI_AMO_DEFINE_ALL(__device__ inline, ishmemx_dev)

#endif /* ISHMEM_AMD_ISHMEMX_DEVICE_H */
