// HIP version of the reference's examples/3_library_apis.cpp with its whole test kernel: the put /
// get ring, barriers, broadcast, atomic fetch-add and XOR, sum reduction, and every thread's atomic
// increment followed by the leader's wait_until — each device call exactly as the reference makes it:
//     ishmem_putmem_nbi(...);                           ishmemx_getmem_nbi_work_group(..., grp);
//     if (grp.leader()) ishmem_barrier_all();           ishmemx_barrier_all_work_group(grp);
//     if (grp.leader()) ishmem_broadcastmem(...);       ishmemx_broadcastmem_work_group(..., grp);
//     *fadd_ret = ishmem_int32_atomic_fetch_add(dst_fadd, fadd_val, next_pe);
//     ishmem_int32_atomic_xor(dst_xor, xor_val, 0);
//     if (grp.leader()) ishmem_int_sum_reduce(...);     ishmemx_int_sum_reduce_work_group(..., grp);
//     ishmem_int_atomic_inc(dst_wait, next_pe);
//     if (grp.leader()) ishmem_int_wait_until(dst_wait, ISHMEM_CMP_GE, num_threads);
// SYCL's nd_item / group become HIP's cooperative groups (grp = this_thread_block(),
// grp.leader() -> grp.thread_rank() == 0, sycl::group_barrier -> grp.sync()).  The host checks are
// the reference's own.  examples/library_apis.hip is the same program without the RMA and AMO lines.
#include <hip/hip_cooperative_groups.h>
#include <hip/hip_runtime.h>

#include <cstdio>
#include <iostream>

#include <ishmem.h>
#include <ishmemx.h>

namespace cg = cooperative_groups;

constexpr int array_size = 10;  // num_threads = array_size / chunk_size
constexpr int chunk_size = 2;   // elements each thread puts
constexpr int32_t fadd_val = 5, xor_val = 2, xor_init = 3;

__global__ void init_kernel(int my_pe, int *src, int *src_bcast, int *reduce_src, int32_t *dst_fadd, int32_t *dst_xor)
{
    dst_fadd[0] = my_pe;
    reduce_src[0] = my_pe;
    dst_xor[0] = xor_init;
    for (int i = 0; i < array_size; i++) src[i] = (my_pe + 1) * (1 << i);  // PE0: 1, 2, 4, ...; PE1: 2, 4, 8, ...
    if (my_pe == 0) src_bcast[0] = 42;
}

__global__ void test_kernel(int *src, int *dst_put, int *dst_get, int32_t *dst_fadd, int32_t *dst_xor, int *dst_sum,
                            int *dst_wait, int *src_bcast, int *dst_bcast, int *fadd_ret, int *reduce_src, int num_threads)
{
    const int my_dev_pe = ishmem_my_pe();
    const int my_dev_npes = ishmem_n_pes();
    auto grp = cg::this_thread_block();
    const size_t i = grp.thread_rank();
    const int next_pe = (my_dev_pe + 1) % my_dev_npes;
    const int prev_pe = my_dev_pe == 0 ? my_dev_npes - 1 : my_dev_pe - 1;

    // put ring: every thread puts its chunk; get ring: the whole group gets the array
    ishmem_putmem_nbi(&dst_put[i * chunk_size], &src[i * chunk_size], sizeof(int) * chunk_size, next_pe);
    ishmemx_getmem_nbi_work_group(dst_get, src, sizeof(int) * array_size, prev_pe, grp);

    grp.sync();
    if (grp.thread_rank() == 0) ishmem_barrier_all();
    grp.sync();
    ishmemx_barrier_all_work_group(grp);

    if (grp.thread_rank() == 0) ishmem_broadcastmem(dst_bcast, src_bcast, sizeof(int), 0);
    ishmemx_broadcastmem_work_group(dst_bcast, src_bcast, sizeof(int), 0, grp);

    *fadd_ret = ishmem_int32_atomic_fetch_add(dst_fadd, fadd_val, next_pe);
    ishmem_int32_atomic_xor(dst_xor, xor_val, 0);

    ishmemx_barrier_all_work_group(grp);

    if (grp.thread_rank() == 0) ishmem_int_sum_reduce(dst_sum, reduce_src, 1);
    ishmemx_int_sum_reduce_work_group(dst_sum, reduce_src, 1, grp);

    // every thread increments dst_wait on the next PE; the leader waits for this PE's own
    ishmem_int_atomic_inc(dst_wait, next_pe);
    if (grp.thread_rank() == 0) ishmem_int_wait_until(dst_wait, ISHMEM_CMP_GE, num_threads);
}

__global__ void verify_kernel(int my_pe, int npes, int num_threads, const int *dst_put, const int *dst_get,
                              const int *dst_bcast, const int32_t *dst_xor, const int32_t *dst_fadd, const int *dst_sum,
                              int *errors)
{
    const int init_val = my_pe == 0 ? npes : my_pe;
    for (int i = 0; i < array_size; i++) {
        if (dst_put[i] != dst_get[i] || dst_put[i] != init_val * (1 << i)) {
            *errors = *errors + 1;
            break;
        }
    }
    if (*dst_bcast != 42) *errors = *errors + 1;
    if (my_pe == 0) {
        int xor_expected = xor_init;
        for (int i = 0; i < npes * num_threads; i++) xor_expected ^= xor_val;
        if (*dst_xor != xor_expected) *errors = *errors + 1;
    }
    if (*dst_fadd != my_pe + fadd_val * num_threads) *errors = *errors + 1;
    if (my_pe == 0 && *dst_sum != npes * (npes - 1) / 2) *errors = *errors + 1;
}

int main()
{
    int dev = 0;
    hipDeviceProp_t prop;
    (void) hipGetDevice(&dev);
    (void) hipGetDeviceProperties(&prop, dev);
    std::cout << "Selected device: " << prop.name << std::endl;

    ishmem_init();
    const int my_pe = ishmem_my_pe();
    const int npes = ishmem_n_pes();
    std::cout << "Hello from PE " << my_pe << std::endl;
    const int num_threads = array_size / chunk_size;

    int *src = (int *) ishmem_malloc(array_size * sizeof(int));
    int *dst_put = (int *) ishmem_calloc(array_size, sizeof(int));
    int *dst_get = (int *) ishmem_calloc(array_size, sizeof(int));
    int32_t *dst_fadd = (int32_t *) ishmem_calloc(1, sizeof(int32_t));
    int32_t *dst_xor = (int32_t *) ishmem_calloc(1, sizeof(int32_t));
    int *dst_sum = (int *) ishmem_calloc(1, sizeof(int));
    int *dst_wait = (int *) ishmem_calloc(1, sizeof(int));
    int *src_bcast = (int *) ishmem_malloc(sizeof(int));
    int *dst_bcast = (int *) ishmem_malloc(sizeof(int));
    int *fadd_ret = (int *) ishmem_calloc(1, sizeof(int));
    int *reduce_src = (int *) ishmem_calloc(1, sizeof(int));

    int *errors = nullptr;  // host memory the kernels can write (sycl::malloc_host)
    if (hipHostMalloc((void **) &errors, sizeof(int), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
        return 1;
    *errors = 0;

    hipLaunchKernelGGL(init_kernel, dim3(1), dim3(1), 0, 0, my_pe, src, src_bcast, reduce_src, dst_fadd, dst_xor);
    (void) hipDeviceSynchronize();
    ishmem_barrier_all();

    hipLaunchKernelGGL(test_kernel, dim3(1), dim3(num_threads), 0, 0, src, dst_put, dst_get, dst_fadd, dst_xor, dst_sum,
                       dst_wait, src_bcast, dst_bcast, fadd_ret, reduce_src, num_threads);
    (void) hipDeviceSynchronize();
    ishmem_barrier_all();

    hipLaunchKernelGGL(verify_kernel, dim3(1), dim3(1), 0, 0, my_pe, npes, num_threads, dst_put, dst_get, dst_bcast,
                       dst_xor, dst_fadd, dst_sum, errors);
    (void) hipDeviceSynchronize();

    if (*errors == 0) std::cout << "PE#" << my_pe << " SUCCESS - verified put/get/amo/broadcast/reduce/sync" << std::endl;
    else std::cout << "PE#" << my_pe << " FAILURE - Error count: " << *errors << std::endl;
    const int nerr = *errors;

    ishmem_free(src);
    ishmem_free(dst_put);
    ishmem_free(dst_get);
    ishmem_free(dst_fadd);
    ishmem_free(dst_xor);
    ishmem_free(dst_sum);
    ishmem_free(dst_wait);
    ishmem_free(src_bcast);
    ishmem_free(dst_bcast);
    ishmem_free(fadd_ret);
    ishmem_free(reduce_src);
    (void) hipHostFree(errors);
    ishmem_finalize();
    return nerr ? 1 : 0;
}
