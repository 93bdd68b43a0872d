/* ishmem_amd — extension API of the reduction path (reference: src/ishmemx.h).
 *
 * The reference's queue-ordered variant
 *   sycl::event ishmemx_<TYPENAME>_<op>_reduce_on_queue([team,] dest, source, nreduce, int *ret,
 *                                                       sycl::queue &q, deps = {})
 * (src/ishmemx.h:1172-1803, src/collectives/reduce_impl.h:444-474) becomes the HIP-stream
 * variant below: enqueue on `stream`, return immediately (0 = enqueued); *ret (device-visible
 * int, may be nullptr) is zeroed in stream order at the call's start and set nonzero by any of the
 * call's launches that fails, so it reads 0 after completion exactly when the call succeeded.
 * The reference's `deps` and returned sycl::event map to the overloads taking
 * (const hipEvent_t *deps, size_t ndeps, hipEvent_t done): the call waits for every dep and
 * records `done` (if not NULL) after its last launch.
 */
#ifndef ISHMEM_AMD_ISHMEMX_H
#define ISHMEM_AMD_ISHMEMX_H

#include "ishmem.h"

#define ISHMEMX_TEAM_NODE ISHMEMI_C_TEAM_NODE /* src/ishmemx.h:11 */

/* After a device-side timeout, all PEs agree on the teams' epochs again (collective over all PEs;
 * no reference counterpart — the reference aborts, src/proxy.cpp:79-84). */
inline int ishmemx_resync(void) { return ishmemi_c_resync(); }

#ifndef __HIP__
typedef struct ihipStream_t *hipStream_t; /* identical to HIP's own typedefs */
typedef struct ihipEvent_t *hipEvent_t;
#endif

namespace ishmemi_cxx {
template <typename T>
inline int reduce_on_stream(ishmem_team_t team, int op, T *dest, const T *source, size_t nreduce,
                            int *ret, hipStream_t stream)
{
    return ishmemi_c_reduce_on_stream(team, op, dtype_of<T>(), (void *) dest, (const void *) source,
                                      nreduce, ret, (void *) stream);
}
template <typename T>
inline int reduce_on_stream(ishmem_team_t team, int op, T *dest, const T *source, size_t nreduce,
                            int *ret, hipStream_t stream, const hipEvent_t *deps, size_t ndeps,
                            hipEvent_t done)
{
    return ishmemi_c_reduce_on_stream_deps(team, op, dtype_of<T>(), (void *) dest,
                                           (const void *) source, nreduce, ret, (void *) stream,
                                           (void *const *) deps, ndeps, (void *) done);
}
}  // namespace ishmemi_cxx

/* Generic forms, as the reference's template <typename T> ishmemx_<op>_reduce_on_queue
 * (src/ishmemx.h:1173, :1191 and the same for every op). */
#define ISHMEMI_CXX_GENERIC_ON_STREAM(OPNAME, OPC)                                                  \
    template <typename T>                                                                          \
    inline int ishmemx_##OPNAME##_reduce_on_stream(T *dest, const T *source, size_t nreduce,        \
                                                   int *ret, hipStream_t stream)                   \
    {                                                                                              \
        return ishmemi_cxx::reduce_on_stream<T>(ISHMEM_TEAM_WORLD, OPC, dest, source, nreduce, ret, \
                                                stream);                                           \
    }                                                                                              \
    template <typename T>                                                                          \
    inline int ishmemx_##OPNAME##_reduce_on_stream(ishmem_team_t team, T *dest, const T *source,    \
                                                   size_t nreduce, int *ret, hipStream_t stream)   \
    {                                                                                              \
        return ishmemi_cxx::reduce_on_stream<T>(team, OPC, dest, source, nreduce, ret, stream);     \
    }                                                                                              \
    template <typename T>                                                                          \
    inline int ishmemx_##OPNAME##_reduce_on_stream(ishmem_team_t team, T *dest, const T *source,    \
                                                   size_t nreduce, int *ret, hipStream_t stream,   \
                                                   const hipEvent_t *deps, size_t ndeps,           \
                                                   hipEvent_t done)                                \
    {                                                                                              \
        return ishmemi_cxx::reduce_on_stream<T>(team, OPC, dest, source, nreduce, ret, stream,      \
                                                deps, ndeps, done);                                \
    }

ISHMEMI_CXX_GENERIC_ON_STREAM(and, ISHMEMI_OP_AND)
ISHMEMI_CXX_GENERIC_ON_STREAM(or, ISHMEMI_OP_OR)
ISHMEMI_CXX_GENERIC_ON_STREAM(xor, ISHMEMI_OP_XOR)
ISHMEMI_CXX_GENERIC_ON_STREAM(max, ISHMEMI_OP_MAX)
ISHMEMI_CXX_GENERIC_ON_STREAM(min, ISHMEMI_OP_MIN)
ISHMEMI_CXX_GENERIC_ON_STREAM(sum, ISHMEMI_OP_SUM)
ISHMEMI_CXX_GENERIC_ON_STREAM(prod, ISHMEMI_OP_PROD)

#define ISHMEMI_CXX_ON_STREAM(TYPENAME, TYPE, OPNAME, OPC)                                          \
    inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_on_stream(                                   \
        TYPE *dest, const TYPE *source, size_t nreduce, int *ret, hipStream_t stream)              \
    {                                                                                              \
        return ishmemi_cxx::reduce_on_stream<TYPE>(ISHMEM_TEAM_WORLD, OPC, dest, source, nreduce,  \
                                                   ret, stream);                                   \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_on_stream(                                   \
        ishmem_team_t team, TYPE *dest, const TYPE *source, size_t nreduce, int *ret,              \
        hipStream_t stream)                                                                        \
    {                                                                                              \
        return ishmemi_cxx::reduce_on_stream<TYPE>(team, OPC, dest, source, nreduce, ret, stream); \
    }                                                                                              \
    /* the reference's `deps` / returned event: wait for deps[0..ndeps), then record `done` */     \
    inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_on_stream(                                   \
        ishmem_team_t team, TYPE *dest, const TYPE *source, size_t nreduce, int *ret,              \
        hipStream_t stream, const hipEvent_t *deps, size_t ndeps, hipEvent_t done)                 \
    {                                                                                              \
        return ishmemi_cxx::reduce_on_stream<TYPE>(team, OPC, dest, source, nreduce, ret, stream,  \
                                                   deps, ndeps, done);                             \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_##OPNAME##_reduce_on_stream(                                   \
        TYPE *dest, const TYPE *source, size_t nreduce, int *ret, hipStream_t stream,              \
        const hipEvent_t *deps, size_t ndeps, hipEvent_t done)                                     \
    {                                                                                              \
        return ishmemi_cxx::reduce_on_stream<TYPE>(ISHMEM_TEAM_WORLD, OPC, dest, source, nreduce,  \
                                                   ret, stream, deps, ndeps, done);                \
    }

ISHMEMI_CXX_BITWISE_TYPES(ISHMEMI_CXX_ON_STREAM, and, ISHMEMI_OP_AND)
ISHMEMI_CXX_BITWISE_TYPES(ISHMEMI_CXX_ON_STREAM, or, ISHMEMI_OP_OR)
ISHMEMI_CXX_BITWISE_TYPES(ISHMEMI_CXX_ON_STREAM, xor, ISHMEMI_OP_XOR)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_ON_STREAM, max, ISHMEMI_OP_MAX)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_ON_STREAM, min, ISHMEMI_OP_MIN)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_ON_STREAM, sum, ISHMEMI_OP_SUM)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_ON_STREAM, prod, ISHMEMI_OP_PROD)

/* Extension (no reference counterpart): reductions of IEEE binary16 ("half") and bfloat16 arrays,
 *   int ishmemx_{half,bfloat16}_{max,min,sum,prod}_reduce([team,] dest, source, nreduce)
 *   int ishmemx_{half,bfloat16}_{max,min,sum,prod}_reduce_on_stream([team,] dest, source, nreduce,
 *                                                                   ret, stream[, deps, ndeps, done])
 * on ishmemx_half_t / ishmemx_bfloat16_t (ishmem.h).  Per element the result is the team-order
 * fold acc = x_0; acc = round_to_nearest_even_T(f32(acc) OP f32(x_j)), rounded after every step
 * (DESIGN.md §3g).  The generic ishmem_<op>_reduce<T> / ishmemx_<op>_reduce_on_stream<T> take the
 * same two types and, under hipcc, _Float16, __half, __bf16 and __hip_bfloat16.  Not for scans,
 * AMOs or waits: those refuse the types. */
#define ISHMEMI_CXX_FP16_BLOCKING(TYPENAME, TYPE, OPNAME, OPC)                                      \
    inline int ishmemx_##TYPENAME##_##OPNAME##_reduce(TYPE *dest, const TYPE *source,              \
                                                      size_t nreduce)                              \
    {                                                                                              \
        return ishmemi_cxx::reduce<TYPE>(ISHMEM_TEAM_WORLD, OPC, dest, source, nreduce);           \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_##OPNAME##_reduce(ishmem_team_t team, TYPE *dest,              \
                                                      const TYPE *source, size_t nreduce)          \
    {                                                                                              \
        return ishmemi_cxx::reduce<TYPE>(team, OPC, dest, source, nreduce);                        \
    }
#define ISHMEMI_CXX_FP16_TYPES(X, OPNAME, OPC)                                                      \
    X(half, ishmemx_half_t, OPNAME, OPC)                                                           \
    X(bfloat16, ishmemx_bfloat16_t, OPNAME, OPC)

ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_FP16_BLOCKING, max, ISHMEMI_OP_MAX)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_FP16_BLOCKING, min, ISHMEMI_OP_MIN)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_FP16_BLOCKING, sum, ISHMEMI_OP_SUM)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_FP16_BLOCKING, prod, ISHMEMI_OP_PROD)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_ON_STREAM, max, ISHMEMI_OP_MAX)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_ON_STREAM, min, ISHMEMI_OP_MIN)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_ON_STREAM, sum, ISHMEMI_OP_SUM)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_ON_STREAM, prod, ISHMEMI_OP_PROD)

/* Extension (no reference counterpart): reduce-scatter, the first half of what a large reduce does
 * (DESIGN.md §3h),
 *   int ishmemx_<TN>_<op>_reduce_scatter([team,] dest, source, nreduce)
 *   int ishmemx_<TN>_<op>_reduce_scatter_on_stream([team,] dest, source, nreduce, ret, stream
 *                                                  [, deps, ndeps, done])
 * and the generic ishmemx_<op>_reduce_scatter<T> / ishmemx_<op>_reduce_scatter_on_stream<T>, for the
 * (op, TYPENAME) pairs of ishmem_<TN>_<op>_reduce plus half and bfloat16 × max / min / sum / prod.
 * source: p blocks of nreduce elements in the symmetric heap (alltoall's source layout).  On member k
 * of a team of p, dest[i] = source_0[k*nreduce + i] OP ... OP source_{p-1}[k*nreduce + i], folded in
 * team order: bit for bit elements [k*nreduce, (k+1)*nreduce) of what the reduce over p*nreduce
 * elements leaves in dest.  dest: nreduce elements of heap, device or pinned host memory, not
 * overlapping the member's own source.  On return (completion of the stream work) dest is final and
 * source may be rewritten. */
namespace ishmemi_cxx {
template <typename T>
inline int reduce_scatter(ishmem_team_t team, int op, T *dest, const T *source, size_t nreduce)
{
    return ishmemi_c_reduce_scatter(team, op, dtype_of<T>(), (void *) dest, (const void *) source, nreduce);
}
template <typename T>
inline int reduce_scatter_on_stream(ishmem_team_t team, int op, T *dest, const T *source, size_t nreduce,
                                    int *ret, hipStream_t stream)
{
    return ishmemi_c_reduce_scatter_on_stream(team, op, dtype_of<T>(), (void *) dest, (const void *) source,
                                              nreduce, ret, (void *) stream);
}
template <typename T>
inline int reduce_scatter_on_stream(ishmem_team_t team, int op, T *dest, const T *source, size_t nreduce,
                                    int *ret, hipStream_t stream, const hipEvent_t *deps, size_t ndeps,
                                    hipEvent_t done)
{
    return ishmemi_c_reduce_scatter_on_stream_deps(team, op, dtype_of<T>(), (void *) dest, (const void *) source,
                                                   nreduce, ret, (void *) stream, (void *const *) deps, ndeps,
                                                   (void *) done);
}
}  // namespace ishmemi_cxx

#define ISHMEMI_CXX_RS_FORMS(TEMPLATE, PREFIX, TYPE, OPC)                                           \
    TEMPLATE inline int PREFIX##_reduce_scatter(TYPE *dest, const TYPE *source, size_t nreduce)    \
    {                                                                                              \
        return ishmemi_cxx::reduce_scatter<TYPE>(ISHMEM_TEAM_WORLD, OPC, dest, source, nreduce);   \
    }                                                                                              \
    TEMPLATE inline int PREFIX##_reduce_scatter(ishmem_team_t team, TYPE *dest, const TYPE *source, \
                                                size_t nreduce)                                    \
    {                                                                                              \
        return ishmemi_cxx::reduce_scatter<TYPE>(team, OPC, dest, source, nreduce);                \
    }                                                                                              \
    TEMPLATE inline int PREFIX##_reduce_scatter_on_stream(TYPE *dest, const TYPE *source,          \
                                                          size_t nreduce, int *ret,                \
                                                          hipStream_t stream)                      \
    {                                                                                              \
        return ishmemi_cxx::reduce_scatter_on_stream<TYPE>(ISHMEM_TEAM_WORLD, OPC, dest, source,   \
                                                           nreduce, ret, stream);                  \
    }                                                                                              \
    TEMPLATE inline int PREFIX##_reduce_scatter_on_stream(ishmem_team_t team, TYPE *dest,          \
                                                          const TYPE *source, size_t nreduce,      \
                                                          int *ret, hipStream_t stream)            \
    {                                                                                              \
        return ishmemi_cxx::reduce_scatter_on_stream<TYPE>(team, OPC, dest, source, nreduce, ret,  \
                                                           stream);                                \
    }                                                                                              \
    TEMPLATE inline int PREFIX##_reduce_scatter_on_stream(TYPE *dest, const TYPE *source,          \
                                                          size_t nreduce, int *ret,                \
                                                          hipStream_t stream,                      \
                                                          const hipEvent_t *deps, size_t ndeps,    \
                                                          hipEvent_t done)                         \
    {                                                                                              \
        return ishmemi_cxx::reduce_scatter_on_stream<TYPE>(ISHMEM_TEAM_WORLD, OPC, dest, source,   \
                                                           nreduce, ret, stream, deps, ndeps,      \
                                                           done);                                  \
    }                                                                                              \
    TEMPLATE inline int PREFIX##_reduce_scatter_on_stream(ishmem_team_t team, TYPE *dest,          \
                                                          const TYPE *source, size_t nreduce,      \
                                                          int *ret, hipStream_t stream,            \
                                                          const hipEvent_t *deps, size_t ndeps,    \
                                                          hipEvent_t done)                         \
    {                                                                                              \
        return ishmemi_cxx::reduce_scatter_on_stream<TYPE>(team, OPC, dest, source, nreduce, ret,  \
                                                           stream, deps, ndeps, done);             \
    }
#define ISHMEMI_CXX_RS_GENERIC(OPNAME, OPC) ISHMEMI_CXX_RS_FORMS(template <typename T>, ishmemx_##OPNAME, T, OPC)
#define ISHMEMI_CXX_RS_TYPED(TYPENAME, TYPE, OPNAME, OPC) \
    ISHMEMI_CXX_RS_FORMS(, ishmemx_##TYPENAME##_##OPNAME, TYPE, OPC)

ISHMEMI_CXX_RS_GENERIC(and, ISHMEMI_OP_AND)
ISHMEMI_CXX_RS_GENERIC(or, ISHMEMI_OP_OR)
ISHMEMI_CXX_RS_GENERIC(xor, ISHMEMI_OP_XOR)
ISHMEMI_CXX_RS_GENERIC(max, ISHMEMI_OP_MAX)
ISHMEMI_CXX_RS_GENERIC(min, ISHMEMI_OP_MIN)
ISHMEMI_CXX_RS_GENERIC(sum, ISHMEMI_OP_SUM)
ISHMEMI_CXX_RS_GENERIC(prod, ISHMEMI_OP_PROD)
ISHMEMI_CXX_BITWISE_TYPES(ISHMEMI_CXX_RS_TYPED, and, ISHMEMI_OP_AND)
ISHMEMI_CXX_BITWISE_TYPES(ISHMEMI_CXX_RS_TYPED, or, ISHMEMI_OP_OR)
ISHMEMI_CXX_BITWISE_TYPES(ISHMEMI_CXX_RS_TYPED, xor, ISHMEMI_OP_XOR)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_RS_TYPED, max, ISHMEMI_OP_MAX)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_RS_TYPED, min, ISHMEMI_OP_MIN)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_RS_TYPED, sum, ISHMEMI_OP_SUM)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_RS_TYPED, prod, ISHMEMI_OP_PROD)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_RS_TYPED, max, ISHMEMI_OP_MAX)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_RS_TYPED, min, ISHMEMI_OP_MIN)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_RS_TYPED, sum, ISHMEMI_OP_SUM)
ISHMEMI_CXX_FP16_TYPES(ISHMEMI_CXX_RS_TYPED, prod, ISHMEMI_OP_PROD)

/* fcollect / collect / scan on a stream (src/ishmemx.h fcollect/collect/inscan/exscan _on_queue). */
inline int ishmemx_fcollectmem_on_stream(ishmem_team_t team, void *dest, const void *source,
                                         size_t nbytes, int *ret, hipStream_t stream)
{
    return ishmemi_c_fcollect_on_stream(team, dest, source, nbytes, ret, (void *) stream);
}
inline int ishmemx_fcollectmem_on_stream(void *dest, const void *source, size_t nbytes, int *ret,
                                         hipStream_t stream)
{
    return ishmemx_fcollectmem_on_stream(ISHMEM_TEAM_WORLD, dest, source, nbytes, ret, stream);
}

namespace ishmemi_cxx {
/* deps -> call -> done around any stream-ordered call (the reference's _on_queue deps / event). */
template <typename F>
inline int with_events(hipStream_t stream, const hipEvent_t *deps, size_t ndeps, hipEvent_t done, F &&call)
{
    if (ishmemi_c_stream_wait_events((void *) stream, (void *const *) deps, ndeps)) return 1;
    if (call()) return 1;
    return ishmemi_c_stream_record_event((void *) stream, (void *) done);
}
}  // namespace ishmemi_cxx

/* collect with per-PE counts on a stream (src/ishmemx.h collectmem / <TN>_collect _on_queue). */
inline int ishmemx_collectmem_on_stream(ishmem_team_t team, void *dest, const void *source,
                                        size_t nbytes, int *ret, hipStream_t stream)
{
    return ishmemi_c_collect_on_stream(team, dest, source, nbytes, ret, (void *) stream);
}
inline int ishmemx_collectmem_on_stream(void *dest, const void *source, size_t nbytes, int *ret,
                                        hipStream_t stream)
{
    return ishmemx_collectmem_on_stream(ISHMEM_TEAM_WORLD, dest, source, nbytes, ret, stream);
}

#define ISHMEMI_CXX_COLL_ON_STREAM(TYPENAME, TYPE, UNUSED1, UNUSED2)                                 \
    inline int ishmemx_##TYPENAME##_fcollect_on_stream(ishmem_team_t team, TYPE *dest,              \
                                                       const TYPE *source, size_t nelems, int *ret, \
                                                       hipStream_t stream)                          \
    {                                                                                              \
        return ishmemi_c_fcollect_on_stream(team, (void *) dest, (const void *) source,             \
                                            nelems * sizeof(TYPE), ret, (void *) stream);           \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_fcollect_on_stream(TYPE *dest, const TYPE *source,              \
                                                       size_t nelems, int *ret, hipStream_t stream) \
    {                                                                                              \
        return ishmemx_##TYPENAME##_fcollect_on_stream(ISHMEM_TEAM_WORLD, dest, source, nelems,    \
                                                       ret, stream);                               \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_collect_on_stream(ishmem_team_t team, TYPE *dest,               \
                                                      const TYPE *source, size_t nelems, int *ret,  \
                                                      hipStream_t stream)                           \
    {                                                                                              \
        return ishmemi_c_collect_on_stream(team, (void *) dest, (const void *) source,              \
                                           nelems * sizeof(TYPE), ret, (void *) stream);            \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_collect_on_stream(TYPE *dest, const TYPE *source, size_t nelems, \
                                                      int *ret, hipStream_t stream)                 \
    {                                                                                              \
        return ishmemx_##TYPENAME##_collect_on_stream(ISHMEM_TEAM_WORLD, dest, source, nelems, ret, \
                                                      stream);                                     \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_sum_inscan_on_stream(ishmem_team_t team, TYPE *dest,            \
                                                         const TYPE *source, size_t nelems,         \
                                                         int *ret, hipStream_t stream)              \
    {                                                                                              \
        return ishmemi_c_scan_on_stream(team, ishmemi_cxx::dtype_of<TYPE>(), 1, (void *) dest,      \
                                        (const void *) source, nelems, ret, (void *) stream);       \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_sum_inscan_on_stream(TYPE *dest, const TYPE *source,            \
                                                         size_t nelems, int *ret,                   \
                                                         hipStream_t stream)                        \
    {                                                                                              \
        return ishmemx_##TYPENAME##_sum_inscan_on_stream(ISHMEM_TEAM_WORLD, dest, source, nelems,  \
                                                         ret, stream);                             \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_sum_exscan_on_stream(ishmem_team_t team, TYPE *dest,            \
                                                         const TYPE *source, size_t nelems,         \
                                                         int *ret, hipStream_t stream)              \
    {                                                                                              \
        return ishmemi_c_scan_on_stream(team, ishmemi_cxx::dtype_of<TYPE>(), 0, (void *) dest,      \
                                        (const void *) source, nelems, ret, (void *) stream);       \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_sum_exscan_on_stream(TYPE *dest, const TYPE *source,            \
                                                         size_t nelems, int *ret,                   \
                                                         hipStream_t stream)                        \
    {                                                                                              \
        return ishmemx_##TYPENAME##_sum_exscan_on_stream(ISHMEM_TEAM_WORLD, dest, source, nelems,  \
                                                         ret, stream);                             \
    }

ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_COLL_ON_STREAM, _, _)

/* The same four with the reference's deps / returned event (team form). */
#define ISHMEMI_CXX_COLL_ON_STREAM_EV(TYPENAME, TYPE, UNUSED1, UNUSED2)                              \
    inline int ishmemx_##TYPENAME##_fcollect_on_stream(ishmem_team_t team, TYPE *dest,              \
        const TYPE *source, size_t nelems, int *ret, hipStream_t stream, const hipEvent_t *deps,    \
        size_t ndeps, hipEvent_t done)                                                             \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return ishmemx_##TYPENAME##_fcollect_on_stream(team, dest, source, nelems, ret, stream); \
        });                                                                                        \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_collect_on_stream(ishmem_team_t team, TYPE *dest,               \
        const TYPE *source, size_t nelems, int *ret, hipStream_t stream, const hipEvent_t *deps,    \
        size_t ndeps, hipEvent_t done)                                                             \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return ishmemx_##TYPENAME##_collect_on_stream(team, dest, source, nelems, ret, stream); \
        });                                                                                        \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_sum_inscan_on_stream(ishmem_team_t team, TYPE *dest,            \
        const TYPE *source, size_t nelems, int *ret, hipStream_t stream, const hipEvent_t *deps,    \
        size_t ndeps, hipEvent_t done)                                                             \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return ishmemx_##TYPENAME##_sum_inscan_on_stream(team, dest, source, nelems, ret, stream); \
        });                                                                                        \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_sum_exscan_on_stream(ishmem_team_t team, TYPE *dest,            \
        const TYPE *source, size_t nelems, int *ret, hipStream_t stream, const hipEvent_t *deps,    \
        size_t ndeps, hipEvent_t done)                                                             \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return ishmemx_##TYPENAME##_sum_exscan_on_stream(team, dest, source, nelems, ret, stream); \
        });                                                                                        \
    }

ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_COLL_ON_STREAM_EV, _, _)

/* broadcast / team barrier on a stream (src/ishmemx.h:846-954, :2228-2235). */
inline int ishmemx_broadcastmem_on_stream(ishmem_team_t team, void *dest, const void *source, size_t nbytes,
                                          int root, int *ret, hipStream_t stream)
{
    return ishmemi_c_broadcast_on_stream(team, dest, source, nbytes, root, ret, (void *) stream);
}
inline int ishmemx_broadcastmem_on_stream(void *dest, const void *source, size_t nbytes, int root, int *ret,
                                          hipStream_t stream)
{
    return ishmemi_c_broadcast_on_stream(ISHMEM_TEAM_WORLD, dest, source, nbytes, root, ret, (void *) stream);
}
template <typename T>
inline int ishmemx_broadcast_on_stream(ishmem_team_t team, T *dest, const T *source, size_t nelems, int root,
                                       int *ret, hipStream_t stream)
{
    return ishmemi_c_broadcast_on_stream(team, (void *) dest, (const void *) source, nelems * sizeof(T), root, ret,
                                         (void *) stream);
}
template <typename T>
inline int ishmemx_broadcast_on_stream(T *dest, const T *source, size_t nelems, int root, int *ret,
                                       hipStream_t stream)
{
    return ishmemx_broadcast_on_stream(ISHMEM_TEAM_WORLD, dest, source, nelems, root, ret, stream);
}
#define ISHMEMI_CXX_BCAST_ON_STREAM(TYPENAME, TYPE, UNUSED1, UNUSED2)                               \
    inline int ishmemx_##TYPENAME##_broadcast_on_stream(ishmem_team_t team, TYPE *dest,             \
                                                        const TYPE *source, size_t nelems, int root, \
                                                        int *ret, hipStream_t stream)              \
    {                                                                                              \
        return ishmemx_broadcast_on_stream(team, dest, source, nelems, root, ret, stream);         \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_broadcast_on_stream(TYPE *dest, const TYPE *source,             \
                                                        size_t nelems, int root, int *ret,         \
                                                        hipStream_t stream)                        \
    {                                                                                              \
        return ishmemx_broadcast_on_stream(dest, source, nelems, root, ret, stream);               \
    }
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_BCAST_ON_STREAM, _, _)

/* alltoall on a stream (src/ishmemx.h ishmemx_alltoallmem_on_queue / <TN>_alltoall_on_queue), with
 * and without a team, and with the reference's deps / returned event. */
inline int ishmemx_alltoallmem_on_stream(ishmem_team_t team, void *dest, const void *source, size_t nbytes,
                                         int *ret, hipStream_t stream)
{
    return ishmemi_c_alltoall_on_stream(team, dest, source, nbytes, ret, (void *) stream);
}
inline int ishmemx_alltoallmem_on_stream(void *dest, const void *source, size_t nbytes, int *ret, hipStream_t stream)
{
    return ishmemi_c_alltoall_on_stream(ISHMEM_TEAM_WORLD, dest, source, nbytes, ret, (void *) stream);
}
inline int ishmemx_alltoallmem_on_stream(ishmem_team_t team, void *dest, const void *source, size_t nbytes,
                                         int *ret, hipStream_t stream, const hipEvent_t *deps, size_t ndeps,
                                         hipEvent_t done)
{
    return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {
        return ishmemi_c_alltoall_on_stream(team, dest, source, nbytes, ret, (void *) stream);
    });
}
inline int ishmemx_alltoallmem_on_stream(void *dest, const void *source, size_t nbytes, int *ret, hipStream_t stream,
                                         const hipEvent_t *deps, size_t ndeps, hipEvent_t done)
{
    return ishmemx_alltoallmem_on_stream(ISHMEM_TEAM_WORLD, dest, source, nbytes, ret, stream, deps, ndeps, done);
}
template <typename T>
inline int ishmemx_alltoall_on_stream(ishmem_team_t team, T *dest, const T *source, size_t nelems, int *ret,
                                      hipStream_t stream)
{
    return ishmemi_c_alltoall_on_stream(team, (void *) dest, (const void *) source, nelems * sizeof(T), ret,
                                        (void *) stream);
}
template <typename T>
inline int ishmemx_alltoall_on_stream(T *dest, const T *source, size_t nelems, int *ret, hipStream_t stream)
{
    return ishmemx_alltoall_on_stream(ISHMEM_TEAM_WORLD, dest, source, nelems, ret, stream);
}
template <typename T>
inline int ishmemx_alltoall_on_stream(ishmem_team_t team, T *dest, const T *source, size_t nelems, int *ret,
                                      hipStream_t stream, const hipEvent_t *deps, size_t ndeps, hipEvent_t done)
{
    return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {
        return ishmemx_alltoall_on_stream(team, dest, source, nelems, ret, stream);
    });
}
template <typename T>
inline int ishmemx_alltoall_on_stream(T *dest, const T *source, size_t nelems, int *ret, hipStream_t stream,
                                      const hipEvent_t *deps, size_t ndeps, hipEvent_t done)
{
    return ishmemx_alltoall_on_stream(ISHMEM_TEAM_WORLD, dest, source, nelems, ret, stream, deps, ndeps, done);
}
#define ISHMEMI_CXX_A2A_ON_STREAM(TYPENAME, TYPE, UNUSED1, UNUSED2)                                  \
    inline int ishmemx_##TYPENAME##_alltoall_on_stream(ishmem_team_t team, TYPE *dest,              \
                                                       const TYPE *source, size_t nelems, int *ret, \
                                                       hipStream_t stream)                          \
    {                                                                                              \
        return ishmemx_alltoall_on_stream(team, dest, source, nelems, ret, stream);                \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_alltoall_on_stream(TYPE *dest, const TYPE *source,              \
                                                       size_t nelems, int *ret, hipStream_t stream) \
    {                                                                                              \
        return ishmemx_alltoall_on_stream(dest, source, nelems, ret, stream);                      \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_alltoall_on_stream(ishmem_team_t team, TYPE *dest,              \
        const TYPE *source, size_t nelems, int *ret, hipStream_t stream, const hipEvent_t *deps,    \
        size_t ndeps, hipEvent_t done)                                                             \
    {                                                                                              \
        return ishmemx_alltoall_on_stream(team, dest, source, nelems, ret, stream, deps, ndeps, done); \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_alltoall_on_stream(TYPE *dest, const TYPE *source,              \
        size_t nelems, int *ret, hipStream_t stream, const hipEvent_t *deps, size_t ndeps,          \
        hipEvent_t done)                                                                           \
    {                                                                                              \
        return ishmemx_alltoall_on_stream(dest, source, nelems, ret, stream, deps, ndeps, done);   \
    }
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_A2A_ON_STREAM, _, _)
inline int ishmemx_team_sync_on_stream(ishmem_team_t team, int *ret, hipStream_t stream)
{
    return ishmemi_c_team_sync_on_stream(team, ret, (void *) stream);
}
inline int ishmemx_sync_all_on_stream(hipStream_t stream)
{
    return ishmemi_c_team_sync_on_stream(ISHMEM_TEAM_WORLD, nullptr, (void *) stream);
}
/* barrier_all = quiet + sync_all; stream order already completes the stream's earlier work. */
inline int ishmemx_barrier_all_on_stream(hipStream_t stream)
{
    return ishmemi_c_team_sync_on_stream(ISHMEM_TEAM_WORLD, nullptr, (void *) stream);
}

/* put / get on a stream (ishmemx_*_{put,get}[_nbi]_on_queue, src/ishmemx.h): enqueued on `stream`,
 * which orders them, so the _nbi form coincides with the plain one; with the reference's deps /
 * returned event as (deps, ndeps, done).  ishmemx_quiet_on_stream: `stream` waits for every host
 * _nbi put / get issued so far. */
#define ISHMEMI_CXX_RMA_ON_STREAM_MEM(NAME, CALL, MUL)                                              \
    inline int ishmemx_##NAME##_on_stream(void *dest, const void *source, size_t n, int pe, hipStream_t stream) \
    {                                                                                              \
        return CALL(dest, source, n * (MUL), pe, (void *) stream);                                 \
    }                                                                                              \
    inline int ishmemx_##NAME##_on_stream(void *dest, const void *source, size_t n, int pe, hipStream_t stream, \
                                          const hipEvent_t *deps, size_t ndeps, hipEvent_t done)   \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done,                                 \
                                        [&] { return CALL(dest, source, n * (MUL), pe, (void *) stream); }); \
    }
#define ISHMEMI_CXX_RMA_ON_STREAM_BOTH(SUFFIX, MUL)                                                 \
    ISHMEMI_CXX_RMA_ON_STREAM_MEM(put##SUFFIX, ishmemi_c_put_on_stream, MUL)                        \
    ISHMEMI_CXX_RMA_ON_STREAM_MEM(get##SUFFIX, ishmemi_c_get_on_stream, MUL)                        \
    ISHMEMI_CXX_RMA_ON_STREAM_MEM(put##SUFFIX##_nbi, ishmemi_c_put_on_stream, MUL)                  \
    ISHMEMI_CXX_RMA_ON_STREAM_MEM(get##SUFFIX##_nbi, ishmemi_c_get_on_stream, MUL)
ISHMEMI_CXX_RMA_ON_STREAM_BOTH(mem, 1)
ISHMEMI_CXX_RMA_ON_STREAM_BOTH(8, 1)
ISHMEMI_CXX_RMA_ON_STREAM_BOTH(16, 2)
ISHMEMI_CXX_RMA_ON_STREAM_BOTH(32, 4)
ISHMEMI_CXX_RMA_ON_STREAM_BOTH(64, 8)
ISHMEMI_CXX_RMA_ON_STREAM_BOTH(128, 16)
#define ISHMEMI_CXX_RMA_ON_STREAM_T(NAME, CALL)                                                     \
    template <typename T>                                                                          \
    inline int ishmemx_##NAME##_on_stream(T *dest, const T *source, size_t nelems, int pe, hipStream_t stream) \
    {                                                                                              \
        return CALL((void *) dest, (const void *) source, nelems * sizeof(T), pe, (void *) stream); \
    }                                                                                              \
    template <typename T>                                                                          \
    inline int ishmemx_##NAME##_on_stream(T *dest, const T *source, size_t nelems, int pe, hipStream_t stream, \
                                          const hipEvent_t *deps, size_t ndeps, hipEvent_t done)   \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return CALL((void *) dest, (const void *) source, nelems * sizeof(T), pe, (void *) stream); \
        });                                                                                        \
    }
ISHMEMI_CXX_RMA_ON_STREAM_T(put, ishmemi_c_put_on_stream)
ISHMEMI_CXX_RMA_ON_STREAM_T(get, ishmemi_c_get_on_stream)
ISHMEMI_CXX_RMA_ON_STREAM_T(put_nbi, ishmemi_c_put_on_stream)
ISHMEMI_CXX_RMA_ON_STREAM_T(get_nbi, ishmemi_c_get_on_stream)
#define ISHMEMI_CXX_RMA_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, NAME)                                   \
    inline int ishmemx_##TYPENAME##_##NAME##_on_stream(TYPE *d, const TYPE *s, size_t n, int pe, hipStream_t st) \
    {                                                                                              \
        return ishmemx_##NAME##_on_stream<TYPE>(d, s, n, pe, st);                                  \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_##NAME##_on_stream(TYPE *d, const TYPE *s, size_t n, int pe, hipStream_t st, \
                                                       const hipEvent_t *deps, size_t ndeps, hipEvent_t done) \
    {                                                                                              \
        return ishmemx_##NAME##_on_stream<TYPE>(d, s, n, pe, st, deps, ndeps, done);               \
    }
#define ISHMEMI_CXX_RMA_ON_STREAM_TYPED(TYPENAME, TYPE, UNUSED1, UNUSED2)                           \
    ISHMEMI_CXX_RMA_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, put)                                        \
    ISHMEMI_CXX_RMA_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, get)                                        \
    ISHMEMI_CXX_RMA_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, put_nbi)                                    \
    ISHMEMI_CXX_RMA_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, get_nbi)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_RMA_ON_STREAM_TYPED, _, _)
/* Blocked put / get (ishmemx_<TN>_ibput / _ibget, src/ishmemx.h:170-197, :389-416): for b < nblocks,
 * `bsize` elements from source + b * sst to dest + b * dst; element strides, >= 1 and >= bsize.
 * Blocking; and the strided / blocked forms on a stream (ishmemx_*_{iput,iget,ibput,ibget}_on_queue,
 * src/ishmemx.h:106-480) with the trailing arguments of ishmemx_<TN>_put_on_stream.  The 128-bit forms
 * count 16-byte elements and 16-byte strides. */
template <typename T>
inline void ishmemx_ibput(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, size_t nblocks, int pe)
{
    (void) ishmemi_c_ibput((void *) dest, (const void *) source, dst, sst, bsize, nblocks, sizeof(T), pe);
}
template <typename T>
inline void ishmemx_ibget(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, size_t nblocks, int pe)
{
    (void) ishmemi_c_ibget((void *) dest, (const void *) source, dst, sst, bsize, nblocks, sizeof(T), pe);
}
/* NAME: iput / iget (CALL with bsize 1) or ibput / ibget; ARGS / PASS: the count arguments. */
#define ISHMEMI_CXX_STRIDED_ON_STREAM_T(NAME, CALL, ARGS, PASS)                                     \
    template <typename T>                                                                          \
    inline int ishmemx_##NAME##_on_stream(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, ARGS, int pe, \
                                          hipStream_t stream)                                      \
    {                                                                                              \
        return CALL((void *) dest, (const void *) source, dst, sst, PASS, sizeof(T), pe, (void *) stream); \
    }                                                                                              \
    template <typename T>                                                                          \
    inline int ishmemx_##NAME##_on_stream(T *dest, const T *source, ptrdiff_t dst, ptrdiff_t sst, ARGS, int pe, \
                                          hipStream_t stream, const hipEvent_t *deps, size_t ndeps, hipEvent_t done) \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return CALL((void *) dest, (const void *) source, dst, sst, PASS, sizeof(T), pe, (void *) stream); \
        });                                                                                        \
    }
#define ISHMEMI_CXX_COMMA ,
ISHMEMI_CXX_STRIDED_ON_STREAM_T(iput, ishmemi_c_ibput_on_stream, size_t nelems, 1 ISHMEMI_CXX_COMMA nelems)
ISHMEMI_CXX_STRIDED_ON_STREAM_T(iget, ishmemi_c_ibget_on_stream, size_t nelems, 1 ISHMEMI_CXX_COMMA nelems)
ISHMEMI_CXX_STRIDED_ON_STREAM_T(ibput, ishmemi_c_ibput_on_stream, size_t bsize ISHMEMI_CXX_COMMA size_t nblocks,
                                bsize ISHMEMI_CXX_COMMA nblocks)
ISHMEMI_CXX_STRIDED_ON_STREAM_T(ibget, ishmemi_c_ibget_on_stream, size_t bsize ISHMEMI_CXX_COMMA size_t nblocks,
                                bsize ISHMEMI_CXX_COMMA nblocks)
#define ISHMEMI_CXX_STRIDED_SIZED_X(BITS)                                                           \
    inline void ishmemx_ibput##BITS(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, size_t nblocks, \
                                    int pe)                                                        \
    {                                                                                              \
        (void) ishmemi_c_ibput(d, s, dst, sst, bsize, nblocks, BITS / 8, pe);                      \
    }                                                                                              \
    inline void ishmemx_ibget##BITS(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, size_t nblocks, \
                                    int pe)                                                        \
    {                                                                                              \
        (void) ishmemi_c_ibget(d, s, dst, sst, bsize, nblocks, BITS / 8, pe);                      \
    }                                                                                              \
    inline int ishmemx_iput##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, int pe, \
                                              hipStream_t st)                                      \
    {                                                                                              \
        return ishmemi_c_ibput_on_stream(d, s, dst, sst, 1, n, BITS / 8, pe, (void *) st);         \
    }                                                                                              \
    inline int ishmemx_iget##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, int pe, \
                                              hipStream_t st)                                      \
    {                                                                                              \
        return ishmemi_c_ibget_on_stream(d, s, dst, sst, 1, n, BITS / 8, pe, (void *) st);         \
    }                                                                                              \
    inline int ishmemx_ibput##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                               size_t nblocks, int pe, hipStream_t st)             \
    {                                                                                              \
        return ishmemi_c_ibput_on_stream(d, s, dst, sst, bsize, nblocks, BITS / 8, pe, (void *) st); \
    }                                                                                              \
    inline int ishmemx_ibget##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                               size_t nblocks, int pe, hipStream_t st)             \
    {                                                                                              \
        return ishmemi_c_ibget_on_stream(d, s, dst, sst, bsize, nblocks, BITS / 8, pe, (void *) st); \
    }                                                                                              \
    inline int ishmemx_iput##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, int pe, \
                                              hipStream_t st, const hipEvent_t *deps, size_t ndeps, hipEvent_t done) \
    {                                                                                              \
        return ishmemi_cxx::with_events(st, deps, ndeps, done, [&] {                               \
            return ishmemi_c_ibput_on_stream(d, s, dst, sst, 1, n, BITS / 8, pe, (void *) st);     \
        });                                                                                        \
    }                                                                                              \
    inline int ishmemx_iget##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, int pe, \
                                              hipStream_t st, const hipEvent_t *deps, size_t ndeps, hipEvent_t done) \
    {                                                                                              \
        return ishmemi_cxx::with_events(st, deps, ndeps, done, [&] {                               \
            return ishmemi_c_ibget_on_stream(d, s, dst, sst, 1, n, BITS / 8, pe, (void *) st);     \
        });                                                                                        \
    }                                                                                              \
    inline int ishmemx_ibput##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                               size_t nblocks, int pe, hipStream_t st, const hipEvent_t *deps, \
                                               size_t ndeps, hipEvent_t done)                      \
    {                                                                                              \
        return ishmemi_cxx::with_events(st, deps, ndeps, done, [&] {                               \
            return ishmemi_c_ibput_on_stream(d, s, dst, sst, bsize, nblocks, BITS / 8, pe, (void *) st); \
        });                                                                                        \
    }                                                                                              \
    inline int ishmemx_ibget##BITS##_on_stream(void *d, const void *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                               size_t nblocks, int pe, hipStream_t st, const hipEvent_t *deps, \
                                               size_t ndeps, hipEvent_t done)                      \
    {                                                                                              \
        return ishmemi_cxx::with_events(st, deps, ndeps, done, [&] {                               \
            return ishmemi_c_ibget_on_stream(d, s, dst, sst, bsize, nblocks, BITS / 8, pe, (void *) st); \
        });                                                                                        \
    }
ISHMEMI_CXX_STRIDED_SIZED_X(8)
ISHMEMI_CXX_STRIDED_SIZED_X(16)
ISHMEMI_CXX_STRIDED_SIZED_X(32)
ISHMEMI_CXX_STRIDED_SIZED_X(64)
ISHMEMI_CXX_STRIDED_SIZED_X(128)
#define ISHMEMI_CXX_STRIDED_TYPED_X(TYPENAME, TYPE, UNUSED1, UNUSED2)                               \
    inline void ishmemx_##TYPENAME##_ibput(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                           size_t nblocks, int pe)                                 \
    {                                                                                              \
        ishmemx_ibput<TYPE>(d, s, dst, sst, bsize, nblocks, pe);                                   \
    }                                                                                              \
    inline void ishmemx_##TYPENAME##_ibget(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                           size_t nblocks, int pe)                                 \
    {                                                                                              \
        ishmemx_ibget<TYPE>(d, s, dst, sst, bsize, nblocks, pe);                                   \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_iput_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, \
                                                   int pe, hipStream_t st)                         \
    {                                                                                              \
        return ishmemx_iput_on_stream<TYPE>(d, s, dst, sst, n, pe, st);                            \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_iget_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, \
                                                   int pe, hipStream_t st)                         \
    {                                                                                              \
        return ishmemx_iget_on_stream<TYPE>(d, s, dst, sst, n, pe, st);                            \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_ibput_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                                    size_t nblocks, int pe, hipStream_t st)        \
    {                                                                                              \
        return ishmemx_ibput_on_stream<TYPE>(d, s, dst, sst, bsize, nblocks, pe, st);              \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_ibget_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                                    size_t nblocks, int pe, hipStream_t st)        \
    {                                                                                              \
        return ishmemx_ibget_on_stream<TYPE>(d, s, dst, sst, bsize, nblocks, pe, st);              \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_iput_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, \
                                                   int pe, hipStream_t st, const hipEvent_t *deps, size_t ndeps, \
                                                   hipEvent_t done)                                \
    {                                                                                              \
        return ishmemx_iput_on_stream<TYPE>(d, s, dst, sst, n, pe, st, deps, ndeps, done);         \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_iget_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t n, \
                                                   int pe, hipStream_t st, const hipEvent_t *deps, size_t ndeps, \
                                                   hipEvent_t done)                                \
    {                                                                                              \
        return ishmemx_iget_on_stream<TYPE>(d, s, dst, sst, n, pe, st, deps, ndeps, done);         \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_ibput_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                                    size_t nblocks, int pe, hipStream_t st, const hipEvent_t *deps, \
                                                    size_t ndeps, hipEvent_t done)                 \
    {                                                                                              \
        return ishmemx_ibput_on_stream<TYPE>(d, s, dst, sst, bsize, nblocks, pe, st, deps, ndeps, done); \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_ibget_on_stream(TYPE *d, const TYPE *s, ptrdiff_t dst, ptrdiff_t sst, size_t bsize, \
                                                    size_t nblocks, int pe, hipStream_t st, const hipEvent_t *deps, \
                                                    size_t ndeps, hipEvent_t done)                 \
    {                                                                                              \
        return ishmemx_ibget_on_stream<TYPE>(d, s, dst, sst, bsize, nblocks, pe, st, deps, ndeps, done); \
    }
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_STRIDED_TYPED_X, _, _)
inline int ishmemx_quiet_on_stream(hipStream_t stream) { return ishmemi_c_quiet_on_stream((void *) stream); }
inline int ishmemx_quiet_on_stream(hipStream_t stream, const hipEvent_t *deps, size_t ndeps, hipEvent_t done)
{
    return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] { return ishmemi_c_quiet_on_stream((void *) stream); });
}

/* Signal operations (ishmemx_signal_set / ishmemx_signal_add, src/ishmemx.h:733-735): one atomic on
 * `pe`'s signal word, blocking. */
inline void ishmemx_signal_set(uint64_t *sig_addr, uint64_t signal, int pe)
{
    (void) ishmemi_c_signal_op(sig_addr, signal, ISHMEM_SIGNAL_SET, pe);
}
inline void ishmemx_signal_add(uint64_t *sig_addr, uint64_t signal, int pe)
{
    (void) ishmemi_c_signal_op(sig_addr, signal, ISHMEM_SIGNAL_ADD, pe);
}

/* put with signal on a stream (ishmemx_*_put_signal[_nbi]_on_queue, src/ishmemx.h:608-738): enqueued
 * on `stream`, which orders it, so the _nbi form coincides with the plain one. */
#define ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_MEM(NAME, MUL)                                             \
    inline int ishmemx_##NAME##_on_stream(void *dest, const void *source, size_t n, uint64_t *sig, uint64_t v, int op, \
                                          int pe, hipStream_t stream)                              \
    {                                                                                              \
        return ishmemi_c_put_signal_on_stream(dest, source, n * (MUL), sig, v, op, pe, (void *) stream); \
    }                                                                                              \
    inline int ishmemx_##NAME##_on_stream(void *dest, const void *source, size_t n, uint64_t *sig, uint64_t v, int op, \
                                          int pe, hipStream_t stream, const hipEvent_t *deps, size_t ndeps,      \
                                          hipEvent_t done)                                         \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return ishmemi_c_put_signal_on_stream(dest, source, n * (MUL), sig, v, op, pe, (void *) stream); \
        });                                                                                        \
    }
#define ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_BOTH(SUFFIX, MUL)                                          \
    ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_MEM(put##SUFFIX##_signal, MUL)                                 \
    ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_MEM(put##SUFFIX##_signal_nbi, MUL)
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_BOTH(mem, 1)
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_BOTH(8, 1)
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_BOTH(16, 2)
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_BOTH(32, 4)
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_BOTH(64, 8)
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_BOTH(128, 16)
#define ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_T(NAME)                                                    \
    template <typename T>                                                                          \
    inline int ishmemx_##NAME##_on_stream(T *dest, const T *source, size_t nelems, uint64_t *sig, uint64_t v, int op, \
                                          int pe, hipStream_t stream)                              \
    {                                                                                              \
        return ishmemi_c_put_signal_on_stream((void *) dest, (const void *) source, nelems * sizeof(T), sig, v, op, pe, \
                                              (void *) stream);                                    \
    }                                                                                              \
    template <typename T>                                                                          \
    inline int ishmemx_##NAME##_on_stream(T *dest, const T *source, size_t nelems, uint64_t *sig, uint64_t v, int op, \
                                          int pe, hipStream_t stream, const hipEvent_t *deps, size_t ndeps,      \
                                          hipEvent_t done)                                         \
    {                                                                                              \
        return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {                           \
            return ishmemi_c_put_signal_on_stream((void *) dest, (const void *) source, nelems * sizeof(T), sig, v, op, \
                                                  pe, (void *) stream);                            \
        });                                                                                        \
    }
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_T(put_signal)
ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_T(put_signal_nbi)
#define ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, NAME)                            \
    inline int ishmemx_##TYPENAME##_##NAME##_on_stream(TYPE *d, const TYPE *s, size_t n, uint64_t *sig, uint64_t v,    \
                                                       int op, int pe, hipStream_t st)             \
    {                                                                                              \
        return ishmemx_##NAME##_on_stream<TYPE>(d, s, n, sig, v, op, pe, st);                      \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_##NAME##_on_stream(TYPE *d, const TYPE *s, size_t n, uint64_t *sig, uint64_t v,    \
                                                       int op, int pe, hipStream_t st, const hipEvent_t *deps,   \
                                                       size_t ndeps, hipEvent_t done)              \
    {                                                                                              \
        return ishmemx_##NAME##_on_stream<TYPE>(d, s, n, sig, v, op, pe, st, deps, ndeps, done);   \
    }
#define ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_TYPED(TYPENAME, TYPE, UNUSED1, UNUSED2)                    \
    ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, put_signal)                          \
    ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_TYPED_ONE(TYPENAME, TYPE, put_signal_nbi)
ISHMEMI_CXX_ARITH_TYPES(ISHMEMI_CXX_PUT_SIGNAL_ON_STREAM_TYPED, _, _)

/* Waits on a stream (ishmemx_<TN>_wait_until_on_queue, ishmemx_signal_wait_until_on_queue,
 * src/ishmemx.h:2011-2040, :2221-2222): `stream` waits until the variable compares true, bounded by
 * the library's timeout.  *ret_value (device-accessible, may be null) receives the value that
 * satisfied the comparison.  Capturable into a graph: the poll target and the compare value are the
 * kernel's frozen arguments.  A timed-out wait shows in ishmemi_c_error_count() (and in `*ret` of
 * ishmemi_c_wait_until_on_stream). */
inline int ishmemx_signal_wait_until_on_stream(uint64_t *sig_addr, int cmp, uint64_t cmp_value, uint64_t *ret_value,
                                               hipStream_t stream)
{
    return ishmemi_c_wait_until_on_stream((void *) sig_addr, ISHMEMI_DT_UINT64, cmp, cmp_value, ret_value, nullptr,
                                          (void *) stream);
}
inline int ishmemx_signal_wait_until_on_stream(uint64_t *sig_addr, int cmp, uint64_t cmp_value, uint64_t *ret_value,
                                               hipStream_t stream, const hipEvent_t *deps, size_t ndeps, hipEvent_t done)
{
    return ishmemi_cxx::with_events(stream, deps, ndeps, done, [&] {
        return ishmemx_signal_wait_until_on_stream(sig_addr, cmp, cmp_value, ret_value, stream);
    });
}
template <typename T>
inline int ishmemx_wait_until_on_stream(T *ivar, int cmp, T cmp_value, hipStream_t stream)
{
    return ishmemi_c_wait_until_on_stream((void *) ivar, ishmemi_cxx::sync_dtype<T>(), cmp, ishmemi_cxx::sync_bits(cmp_value),
                                          nullptr, nullptr, (void *) stream);
}
template <typename T>
inline int ishmemx_wait_until_on_stream(T *ivar, int cmp, T cmp_value, hipStream_t stream, const hipEvent_t *deps,
                                        size_t ndeps, hipEvent_t done)
{
    return ishmemi_cxx::with_events(stream, deps, ndeps, done,
                                    [&] { return ishmemx_wait_until_on_stream<T>(ivar, cmp, cmp_value, stream); });
}
#define ISHMEMI_CXX_SYNC_ON_STREAM_TYPED(TYPENAME, TYPE)                                            \
    inline int ishmemx_##TYPENAME##_wait_until_on_stream(TYPE *ivar, int cmp, TYPE v, hipStream_t st) \
    {                                                                                              \
        return ishmemx_wait_until_on_stream<TYPE>(ivar, cmp, v, st);                               \
    }                                                                                              \
    inline int ishmemx_##TYPENAME##_wait_until_on_stream(TYPE *ivar, int cmp, TYPE v, hipStream_t st,                \
                                                         const hipEvent_t *deps, size_t ndeps, hipEvent_t done)     \
    {                                                                                              \
        return ishmemx_wait_until_on_stream<TYPE>(ivar, cmp, v, st, deps, ndeps, done);            \
    }
ISHMEMI_CXX_SYNC_TYPES(ISHMEMI_CXX_SYNC_ON_STREAM_TYPED)

/* Vector waits on a stream (ishmemx_<TN>_wait_until_all / _any / _some[_vector]_on_queue,
 * src/ishmemx.h:2043-2208; the reference has no test_*_on_queue): `stream` waits, bounded by the
 * library's timeout.  *ret (any: the index, some: the count; may be null), status, cmp_values and
 * indices must be device-accessible: the kernel reads and writes them when it runs, so a captured
 * call reads their contents at every replay.  A timed-out wait shows in ishmemi_c_error_count() (and in
 * `*ret` of ishmemi_c_sync_vector_on_stream).  DESIGN.md §3f. */
namespace ishmemi_cxx {
template <typename T>
inline int sync_vector_on_stream(int mode, T *ivars, size_t nelems, size_t *indices, const int *status, int cmp, T cmp_value,
                                 const T *cmp_values, size_t *ret, hipStream_t stream)
{
    return ishmemi_c_sync_vector_on_stream(mode, sync_dtype<T>(), (void *) ivars, nelems, indices, status, cmp,
                                           sync_bits(cmp_value), (const void *) cmp_values, ret, nullptr, (void *) stream);
}
}  // namespace ishmemi_cxx
/* The three waits of one form, named PREFIX<op>SUFFIX; CV and the trailing arguments: `T v` and
 * `v, nullptr` (scalar), `const T *v` and `T(), v` (_vector). */
#define ISHMEMI_CXX_SYNC_VECTOR_ON_STREAM_FORM(TEMPLATE, PREFIX, SUFFIX, T, MODEBITS, CV, ...)                \
    TEMPLATE inline int PREFIX##wait_until_all##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV, hipStream_t st) \
    {                                                                                              \
        return ishmemi_cxx::sync_vector_on_stream<T>(ISHMEMI_C_SYNC_WAIT_ALL | MODEBITS, ivars, n, nullptr, status, cmp, \
                                                     __VA_ARGS__, nullptr, st);                    \
    }                                                                                              \
    TEMPLATE inline int PREFIX##wait_until_any##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV, size_t *ret, hipStream_t st) \
    {                                                                                              \
        return ishmemi_cxx::sync_vector_on_stream<T>(ISHMEMI_C_SYNC_WAIT_ANY | MODEBITS, ivars, n, nullptr, status, cmp, \
                                                     __VA_ARGS__, ret, st);                        \
    }                                                                                              \
    TEMPLATE inline int PREFIX##wait_until_some##SUFFIX(T *ivars, size_t n, size_t *indices, const int *status, int cmp, CV,   \
                                              size_t *ret, hipStream_t st)                         \
    {                                                                                              \
        return ishmemi_cxx::sync_vector_on_stream<T>(ISHMEMI_C_SYNC_WAIT_SOME | MODEBITS, ivars, n, indices, status, cmp, \
                                                     __VA_ARGS__, ret, st);                        \
    }                                                                                              \
    TEMPLATE inline int PREFIX##wait_until_all##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV, hipStream_t st,     \
                                             const hipEvent_t *deps, size_t ndeps, hipEvent_t done) \
    {                                                                                              \
        return ishmemi_cxx::with_events(st, deps, ndeps, done, [&] { return PREFIX##wait_until_all##SUFFIX(ivars, n, status, cmp, v, st); }); \
    }                                                                                              \
    TEMPLATE inline int PREFIX##wait_until_any##SUFFIX(T *ivars, size_t n, const int *status, int cmp, CV, size_t *ret, hipStream_t st, \
                                             const hipEvent_t *deps, size_t ndeps, hipEvent_t done) \
    {                                                                                              \
        return ishmemi_cxx::with_events(st, deps, ndeps, done,                                     \
                                        [&] { return PREFIX##wait_until_any##SUFFIX(ivars, n, status, cmp, v, ret, st); }); \
    }                                                                                              \
    TEMPLATE inline int PREFIX##wait_until_some##SUFFIX(T *ivars, size_t n, size_t *indices, const int *status, int cmp, CV,   \
                                              size_t *ret, hipStream_t st, const hipEvent_t *deps, size_t ndeps,    \
                                              hipEvent_t done)                                     \
    {                                                                                              \
        return ishmemi_cxx::with_events(st, deps, ndeps, done,                                     \
                                        [&] { return PREFIX##wait_until_some##SUFFIX(ivars, n, indices, status, cmp, v, ret, st); }); \
    }
ISHMEMI_CXX_SYNC_VECTOR_ON_STREAM_FORM(template <typename T>, ishmemx_, _on_stream, T, 0, T v, v, (const T *) nullptr)
ISHMEMI_CXX_SYNC_VECTOR_ON_STREAM_FORM(template <typename T>, ishmemx_, _vector_on_stream, T, ISHMEMI_C_SYNC_VECTOR,
                                       const T *v, T(), v)
#define ISHMEMI_CXX_SYNC_VECTOR_ON_STREAM_TYPED(TYPENAME, TYPE)                                     \
    ISHMEMI_CXX_SYNC_VECTOR_ON_STREAM_FORM(, ishmemx_##TYPENAME##_, _on_stream, TYPE, 0, TYPE v, v,              \
                                           (const TYPE *) nullptr)                                 \
    ISHMEMI_CXX_SYNC_VECTOR_ON_STREAM_FORM(, ishmemx_##TYPENAME##_, _vector_on_stream, TYPE,                     \
                                           ISHMEMI_C_SYNC_VECTOR, const TYPE *v, (TYPE) 0, v)
ISHMEMI_CXX_SYNC_TYPES(ISHMEMI_CXX_SYNC_VECTOR_ON_STREAM_TYPED)

/* Explicit-identity init (the role of ishmemx_init_attr, src/ishmemx.h:21-37). */
inline int ishmemx_init_pe(int pe, int npes, int device, const char *bootstrap_key)
{
    return ishmemi_c_init_pe(pe, npes, device, bootstrap_key);
}

#endif /* ISHMEM_AMD_ISHMEMX_H */
