/* ishmem_amd — generator of the atomic memory operations' names, shared by the host API (ishmem.h)
 * and the device API (ishmemx_device.h): the 22 templates ishmem_atomic_<op>[_nbi]<T> and the 229
 * typed names ishmem_<TYPENAME>_atomic_<op>[_nbi] with the reference's signatures (src/ishmem.h:331-640,
 * src/amo.cpp:93-134, :230-253).  The three type lists are the reference's (src/amo_impl.h:15-37):
 *   BIT  uint ulong ulonglong int32 int64 uint32 uint64          and / or / xor and their fetch forms
 *   STD  BIT + int long longlong size ptrdiff                     compare_swap, inc, add and fetch forms
 *   EXT  STD + float double                                       fetch, set, swap
 * The reference's header also declares 14 schar forms that src/amo.cpp never defines; they are not
 * provided (the precedent of the schar bitwise reduces, ishmem.h's header comment).
 *
 * ISHMEMI_AMO_DEFINE_ALL(QUAL, NS) emits every name with the function qualifier QUAL on top of three
 * functions of namespace NS:
 *   T    NS::amo_f<T>(int op, T *dest, T val, T cond, int pe)            fetching, returns the old value
 *   void NS::amo_v<T>(int op, T *dest, T val, int pe)                    non-fetching
 *   void NS::amo_n<T>(int op, T *fetch, T *dest, T val, T cond, int pe)  _nbi, old value to *fetch
 * with op one of ISHMEMI_C_AMO_*.
 *
 * The templates static_assert their type list, so ishmem_atomic_fetch_add<float> or
 * ishmem_atomic_fetch_and<int> does not compile.  A list is a list of TYPENAMES, and C++ sees only
 * types: where int32_t is int, the template argument `int` (typename int: STD, not BIT) cannot be told
 * from int32_t (BIT), and the bitwise templates refuse it — ishmem_int32_atomic_fetch_and and its kin
 * are the way to a bitwise AMO on an int32_t; every other listed type reaches its templates. */
#ifndef ISHMEM_AMD_ISHMEM_AMO_H
#define ISHMEM_AMD_ISHMEM_AMO_H

#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "ishmem_capi.h"

namespace ishmemi_amo {
template <typename T, typename... Us>
struct in_list : std::false_type {};
template <typename T, typename U, typename... Us>
struct in_list<T, U, Us...> : std::integral_constant<bool, std::is_same<T, U>::value || in_list<T, Us...>::value> {};

template <typename T>
struct is_bit
    : std::integral_constant<bool, in_list<T, unsigned int, unsigned long, unsigned long long, int64_t, uint32_t, uint64_t>::value ||
                                       (std::is_same<T, int32_t>::value && !std::is_same<int32_t, int>::value)> {};
template <typename T>
struct is_std : std::integral_constant<bool, in_list<T, unsigned int, unsigned long, unsigned long long, int32_t, int64_t, uint32_t,
                                                     uint64_t, int, long, long long, size_t, ptrdiff_t>::value> {};
template <typename T>
struct is_ext : std::integral_constant<bool, is_std<T>::value || in_list<T, float, double>::value> {};

/* The C ABI's dtype of an AMO type (every listed type is 4 or 8 bytes wide). */
template <typename T>
constexpr int dtype()
{
    return std::is_same<T, float>::value    ? ISHMEMI_DT_FLOAT
           : std::is_same<T, double>::value ? ISHMEMI_DT_DOUBLE
           : std::is_signed<T>::value       ? (sizeof(T) == 4 ? ISHMEMI_DT_INT32 : ISHMEMI_DT_INT64)
                                            : (sizeof(T) == 4 ? ISHMEMI_DT_UINT32 : ISHMEMI_DT_UINT64);
}
/* The unsigned integer of T's width: what the value travels as. */
template <typename T>
using bits_t = typename std::conditional<sizeof(T) == 8, uint64_t, uint32_t>::type;
}  // namespace ishmemi_amo

#define ISHMEMI_AMO_ASSERT(LIST, WHAT) static_assert(ishmemi_amo::LIST<T>::value, WHAT);

/* One name of each argument shape.  HEAD: `template <typename T> QUAL` or QUAL; T: the type. */
#define ISHMEMI_AMO_F0(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD T NAME(T *dest, int pe) { CHECK typedef T V; return NS::amo_f<V>(OPC, dest, V(), V(), pe); }
#define ISHMEMI_AMO_F1(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD T NAME(T *dest, T val, int pe) { CHECK typedef T V; return NS::amo_f<V>(OPC, dest, val, V(), pe); }
#define ISHMEMI_AMO_F2(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD T NAME(T *dest, T cond, T val, int pe) { CHECK typedef T V; return NS::amo_f<V>(OPC, dest, val, cond, pe); }
#define ISHMEMI_AMO_V0(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD void NAME(T *dest, int pe) { CHECK typedef T V; NS::amo_v<V>(OPC, dest, V(), pe); }
#define ISHMEMI_AMO_V1(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD void NAME(T *dest, T val, int pe) { CHECK typedef T V; NS::amo_v<V>(OPC, dest, val, pe); }
#define ISHMEMI_AMO_N0(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD void NAME(T *fetch, T *dest, int pe) { CHECK typedef T V; NS::amo_n<V>(OPC, fetch, dest, V(), V(), pe); }
#define ISHMEMI_AMO_N1(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD void NAME(T *fetch, T *dest, T val, int pe) { CHECK typedef T V; NS::amo_n<V>(OPC, fetch, dest, val, V(), pe); }
#define ISHMEMI_AMO_N2(HEAD, NAME, T, OPC, NS, CHECK)                                               \
    HEAD void NAME(T *fetch, T *dest, T cond, T val, int pe) { CHECK typedef T V; NS::amo_n<V>(OPC, fetch, dest, val, cond, pe); }

/* The operations of each list: X(shape, name, op code). */
#define ISHMEMI_AMO_EXT_OPS(X, ...)                                                                 \
    X(F0, atomic_fetch, ISHMEMI_C_AMO_FETCH, __VA_ARGS__)                                           \
    X(V1, atomic_set, ISHMEMI_C_AMO_SET, __VA_ARGS__)                                               \
    X(F1, atomic_swap, ISHMEMI_C_AMO_SWAP, __VA_ARGS__)                                             \
    X(N0, atomic_fetch_nbi, ISHMEMI_C_AMO_FETCH, __VA_ARGS__)                                       \
    X(N1, atomic_swap_nbi, ISHMEMI_C_AMO_SWAP, __VA_ARGS__)
#define ISHMEMI_AMO_STD_OPS(X, ...)                                                                 \
    X(F2, atomic_compare_swap, ISHMEMI_C_AMO_COMPARE_SWAP, __VA_ARGS__)                             \
    X(F0, atomic_fetch_inc, ISHMEMI_C_AMO_FETCH_INC, __VA_ARGS__)                                   \
    X(V0, atomic_inc, ISHMEMI_C_AMO_INC, __VA_ARGS__)                                               \
    X(F1, atomic_fetch_add, ISHMEMI_C_AMO_FETCH_ADD, __VA_ARGS__)                                   \
    X(V1, atomic_add, ISHMEMI_C_AMO_ADD, __VA_ARGS__)                                               \
    X(N2, atomic_compare_swap_nbi, ISHMEMI_C_AMO_COMPARE_SWAP, __VA_ARGS__)                         \
    X(N0, atomic_fetch_inc_nbi, ISHMEMI_C_AMO_FETCH_INC, __VA_ARGS__)                               \
    X(N1, atomic_fetch_add_nbi, ISHMEMI_C_AMO_FETCH_ADD, __VA_ARGS__)
#define ISHMEMI_AMO_BIT_OPS(X, ...)                                                                 \
    X(F1, atomic_fetch_and, ISHMEMI_C_AMO_FETCH_AND, __VA_ARGS__)                                   \
    X(F1, atomic_fetch_or, ISHMEMI_C_AMO_FETCH_OR, __VA_ARGS__)                                     \
    X(F1, atomic_fetch_xor, ISHMEMI_C_AMO_FETCH_XOR, __VA_ARGS__)                                   \
    X(V1, atomic_and, ISHMEMI_C_AMO_AND, __VA_ARGS__)                                               \
    X(V1, atomic_or, ISHMEMI_C_AMO_OR, __VA_ARGS__)                                                 \
    X(V1, atomic_xor, ISHMEMI_C_AMO_XOR, __VA_ARGS__)                                               \
    X(N1, atomic_fetch_and_nbi, ISHMEMI_C_AMO_FETCH_AND, __VA_ARGS__)                               \
    X(N1, atomic_fetch_or_nbi, ISHMEMI_C_AMO_FETCH_OR, __VA_ARGS__)                                 \
    X(N1, atomic_fetch_xor_nbi, ISHMEMI_C_AMO_FETCH_XOR, __VA_ARGS__)

/* The typenames of each list (src/amo_impl.h:15-37): X(TYPENAME, TYPE). */
#define ISHMEMI_AMO_BIT_TYPES(X, ...)                                                               \
    X(uint, unsigned int, __VA_ARGS__) X(ulong, unsigned long, __VA_ARGS__)                         \
    X(ulonglong, unsigned long long, __VA_ARGS__) X(int32, int32_t, __VA_ARGS__)                    \
    X(int64, int64_t, __VA_ARGS__) X(uint32, uint32_t, __VA_ARGS__) X(uint64, uint64_t, __VA_ARGS__)
#define ISHMEMI_AMO_STD_ONLY_TYPES(X, ...)                                                          \
    X(int, int, __VA_ARGS__) X(long, long, __VA_ARGS__) X(longlong, long long, __VA_ARGS__)         \
    X(size, size_t, __VA_ARGS__) X(ptrdiff, ptrdiff_t, __VA_ARGS__)
#define ISHMEMI_AMO_EXT_ONLY_TYPES(X, ...) X(float, float, __VA_ARGS__) X(double, double, __VA_ARGS__)

#define ISHMEMI_AMO_GENERIC(SHAPE, NAME, OPC, QUAL, NS, LIST, WHAT)                                 \
    ISHMEMI_AMO_##SHAPE(template <typename T> QUAL, ishmem_##NAME, T, OPC, NS, ISHMEMI_AMO_ASSERT(LIST, "ishmem_" #NAME ": " WHAT))
#define ISHMEMI_AMO_TYPED(SHAPE, NAME, OPC, TYPENAME, TYPE, QUAL, NS)                               \
    ISHMEMI_AMO_##SHAPE(QUAL, ishmem_##TYPENAME##_##NAME, TYPE, OPC, NS, )
#define ISHMEMI_AMO_TYPED_EXT(TYPENAME, TYPE, QUAL, NS) ISHMEMI_AMO_EXT_OPS(ISHMEMI_AMO_TYPED, TYPENAME, TYPE, QUAL, NS)
#define ISHMEMI_AMO_TYPED_STD(TYPENAME, TYPE, QUAL, NS)                                             \
    ISHMEMI_AMO_TYPED_EXT(TYPENAME, TYPE, QUAL, NS) ISHMEMI_AMO_STD_OPS(ISHMEMI_AMO_TYPED, TYPENAME, TYPE, QUAL, NS)
#define ISHMEMI_AMO_TYPED_BIT(TYPENAME, TYPE, QUAL, NS)                                             \
    ISHMEMI_AMO_TYPED_STD(TYPENAME, TYPE, QUAL, NS) ISHMEMI_AMO_BIT_OPS(ISHMEMI_AMO_TYPED, TYPENAME, TYPE, QUAL, NS)

#define ISHMEMI_AMO_DEFINE_ALL(QUAL, NS)                                                            \
    ISHMEMI_AMO_EXT_OPS(ISHMEMI_AMO_GENERIC, QUAL, NS, is_ext, "one of the 14 extended AMO types")  \
    ISHMEMI_AMO_STD_OPS(ISHMEMI_AMO_GENERIC, QUAL, NS, is_std, "one of the 12 standard AMO types (integers)") \
    ISHMEMI_AMO_BIT_OPS(ISHMEMI_AMO_GENERIC, QUAL, NS, is_bit, "one of the 7 bitwise AMO types")    \
    ISHMEMI_AMO_BIT_TYPES(ISHMEMI_AMO_TYPED_BIT, QUAL, NS)                                          \
    ISHMEMI_AMO_STD_ONLY_TYPES(ISHMEMI_AMO_TYPED_STD, QUAL, NS)                                     \
    ISHMEMI_AMO_EXT_ONLY_TYPES(ISHMEMI_AMO_TYPED_EXT, QUAL, NS)

#endif /* ISHMEM_AMD_ISHMEM_AMO_H */
