/* ishmem_amd — the 16-bit floating-point element types of the reduction extension.
 *
 * No reference counterpart: the reference's reductions stop at float / double.  Included by
 * ishmem.h (host names in ishmemx.h) and ishmemx_device.h (device names); DESIGN.md §3g has the
 * arithmetic contract.
 *
 * ishmemx_half_t / ishmemx_bfloat16_t are plain 2-byte storage — `bits` is the IEEE binary16 /
 * bfloat16 encoding — so they compile as C++ anywhere, with no HIP headers.  Under hipcc the
 * compiler's (_Float16, __bf16) and HIP's (__half, __hip_bfloat16) own types are accepted by the
 * generic template forms as well.
 */
#ifndef ISHMEM_AMD_ISHMEMX_FP16_H
#define ISHMEM_AMD_ISHMEMX_FP16_H

#include <stdint.h>

#include <type_traits>

#if defined(__HIP__)
#include <hip/hip_bf16.h>
#include <hip/hip_fp16.h>
#endif

typedef struct {
    uint16_t bits;
} ishmemx_half_t;
typedef struct {
    uint16_t bits;
} ishmemx_bfloat16_t;

namespace ishmemi_cxx {
/* 1: an IEEE binary16 type, 2: a bfloat16 type, 0: neither. */
template <typename T>
constexpr int fp16_kind()
{
    if constexpr (std::is_same_v<T, ishmemx_half_t>) return 1;
    else if constexpr (std::is_same_v<T, ishmemx_bfloat16_t>) return 2;
#if defined(__HIP__)
    else if constexpr (std::is_same_v<T, _Float16> || std::is_same_v<T, __half>) return 1;
    else if constexpr (std::is_same_v<T, __bf16> || std::is_same_v<T, __hip_bfloat16>) return 2;
#endif
    else return 0;
}
}  // namespace ishmemi_cxx

#endif /* ISHMEM_AMD_ISHMEMX_FP16_H */
