/* ishmem_amd - generator of the vector waits' and tests' C++ names (ishmem_<TN>_wait_until_all / _any /
 * _some[_vector], ishmem_<TN>_test_all / _any / _some[_vector] and the templates; src/ishmem.h:1343-1538),
 * shared by the host forms (ishmem.h) and the device forms (ishmemx_device.h), as ishmem_amo.h is for
 * the atomics.  QUAL: `inline` or `__device__ inline`; NS: a namespace with
 *   template <typename T> size_t sync_vector(int mode, T *ivars, size_t nelems, size_t *indices,
 *                                            const int *status, int cmp, T cmp_value, const T *cmp_values);
 * and `kSyncVec` (ISHMEMI_C_SYNC_VECTOR).  DESIGN.md section 3f. */
#ifndef ISHMEM_AMD_ISHMEM_SYNC_H
#define ISHMEM_AMD_ISHMEM_SYNC_H

#include <stddef.h>

#include "ishmem_capi.h"

#define ISHMEMI_SYNC_VECTOR_GENERIC(QUAL, NS)                                                   \
    template <typename T>                                                                          \
    QUAL void ishmem_wait_until_all(T *ivars, size_t nelems, const int *status, int cmp, T cmp_value) \
    {                                                                                              \
        (void) NS::sync_vector<T>(ISHMEMI_C_SYNC_WAIT_ALL, ivars, nelems, nullptr, status, cmp, cmp_value, nullptr); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_wait_until_any(T *ivars, size_t nelems, const int *status, int cmp, T cmp_value) \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_WAIT_ANY, ivars, nelems, nullptr, status, cmp, cmp_value, nullptr); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_wait_until_some(T *ivars, size_t nelems, size_t *indices, const int *status, int cmp, T cmp_value) \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_WAIT_SOME, ivars, nelems, indices, status, cmp, cmp_value, nullptr); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL int ishmem_test_all(T *ivars, size_t nelems, const int *status, int cmp, T cmp_value)      \
    {                                                                                              \
        return (int) NS::sync_vector<T>(ISHMEMI_C_SYNC_TEST_ALL, ivars, nelems, nullptr, status, cmp, cmp_value, nullptr); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_test_any(T *ivars, size_t nelems, const int *status, int cmp, T cmp_value)   \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_TEST_ANY, ivars, nelems, nullptr, status, cmp, cmp_value, nullptr); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_test_some(T *ivars, size_t nelems, size_t *indices, const int *status, int cmp, T cmp_value) \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_TEST_SOME, ivars, nelems, indices, status, cmp, cmp_value, nullptr); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL void ishmem_wait_until_all_vector(T *ivars, size_t nelems, const int *status, int cmp, const T *cmp_values) \
    {                                                                                              \
        (void) NS::sync_vector<T>(ISHMEMI_C_SYNC_WAIT_ALL | NS::kSyncVec, ivars, nelems, nullptr, status, cmp, T(), cmp_values); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_wait_until_any_vector(T *ivars, size_t nelems, const int *status, int cmp, const T *cmp_values) \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_WAIT_ANY | NS::kSyncVec, ivars, nelems, nullptr, status, cmp, T(), cmp_values); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_wait_until_some_vector(T *ivars, size_t nelems, size_t *indices, const int *status, int cmp,    \
                                              const T *cmp_values)                                 \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_WAIT_SOME | NS::kSyncVec, ivars, nelems, indices, status, cmp, T(), cmp_values); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL int ishmem_test_all_vector(T *ivars, size_t nelems, const int *status, int cmp, const T *cmp_values) \
    {                                                                                              \
        return (int) NS::sync_vector<T>(ISHMEMI_C_SYNC_TEST_ALL | NS::kSyncVec, ivars, nelems, nullptr, status, cmp, T(), cmp_values); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_test_any_vector(T *ivars, size_t nelems, const int *status, int cmp, const T *cmp_values) \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_TEST_ANY | NS::kSyncVec, ivars, nelems, nullptr, status, cmp, T(), cmp_values); \
    }                                                                                              \
    template <typename T>                                                                          \
    QUAL size_t ishmem_test_some_vector(T *ivars, size_t nelems, size_t *indices, const int *status, int cmp,          \
                                        const T *cmp_values)                                       \
    {                                                                                              \
        return NS::sync_vector<T>(ISHMEMI_C_SYNC_TEST_SOME | NS::kSyncVec, ivars, nelems, indices, status, cmp, T(), cmp_values); \
    }
/* The 12 operations of one typename; CV is `TYPE v` / `const TYPE *v` of the scalar / _vector forms. */
#define ISHMEMI_SYNC_VECTOR_TYPED_FORM(QUAL, TYPENAME, TYPE, SUFFIX, CV)                        \
    QUAL void ishmem_##TYPENAME##_wait_until_all##SUFFIX(TYPE *ivars, size_t n, const int *status, int cmp, CV) \
    {                                                                                              \
        ishmem_wait_until_all##SUFFIX<TYPE>(ivars, n, status, cmp, v);                             \
    }                                                                                              \
    QUAL size_t ishmem_##TYPENAME##_wait_until_any##SUFFIX(TYPE *ivars, size_t n, const int *status, int cmp, CV) \
    {                                                                                              \
        return ishmem_wait_until_any##SUFFIX<TYPE>(ivars, n, status, cmp, v);                      \
    }                                                                                              \
    QUAL size_t ishmem_##TYPENAME##_wait_until_some##SUFFIX(TYPE *ivars, size_t n, size_t *indices, const int *status, \
                                                            int cmp, CV)                           \
    {                                                                                              \
        return ishmem_wait_until_some##SUFFIX<TYPE>(ivars, n, indices, status, cmp, v);            \
    }                                                                                              \
    QUAL int ishmem_##TYPENAME##_test_all##SUFFIX(TYPE *ivars, size_t n, const int *status, int cmp, CV) \
    {                                                                                              \
        return ishmem_test_all##SUFFIX<TYPE>(ivars, n, status, cmp, v);                            \
    }                                                                                              \
    QUAL size_t ishmem_##TYPENAME##_test_any##SUFFIX(TYPE *ivars, size_t n, const int *status, int cmp, CV) \
    {                                                                                              \
        return ishmem_test_any##SUFFIX<TYPE>(ivars, n, status, cmp, v);                            \
    }                                                                                              \
    QUAL size_t ishmem_##TYPENAME##_test_some##SUFFIX(TYPE *ivars, size_t n, size_t *indices, const int *status,      \
                                                      int cmp, CV)                                 \
    {                                                                                              \
        return ishmem_test_some##SUFFIX<TYPE>(ivars, n, indices, status, cmp, v);                  \
    }
#endif /* ISHMEM_AMD_ISHMEM_SYNC_H */
