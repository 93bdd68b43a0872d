// HIP version of the reference's examples/2_get.cpp: every PE fills a symmetric array with its own
// PE number, then a kernel reads the next PE's array element by element with the device call,
// unchanged from the reference:
//     dst[id] = ishmem_int_g(&src[id], next_pe)
// Only the SYCL parts differ: q.parallel_for becomes a HIP kernel launch, sycl::malloc_host becomes
// hipHostMalloc.  The program checks what it received and prints SUCCESS / FAILURE.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <iostream>

#include <ishmem.h>
#include <ishmemx.h>

constexpr size_t N = 10;

__global__ void fill(int *src, int my_pe)
{
    const size_t id = threadIdx.x;
    if (id < N) src[id] = my_pe;
}

__global__ void get_from_next(int *dst, int *src, int my_pe, int npes)
{
    const size_t id = threadIdx.x;
    if (id >= N) return;
    int next_pe = (my_pe + 1) % npes;
    dst[id] = ishmem_int_g(&src[id], next_pe);
}

__global__ void verify(const int *dst, int *check, int my_pe, int npes)
{
    const size_t id = threadIdx.x;
    if (id >= N) return;
    int expected = (my_pe + 1) % npes;
    check[id] = dst[id] != expected ? 1 : 0;
}

int main()
{
    // Initialize ISHMEM
    ishmem_init();

    // Each PE is mapped to a device.
    int my_pe = ishmem_my_pe();
    // Get total number of PEs
    int npes = ishmem_n_pes();

    hipDeviceProp_t prop;
    int dev = 0;
    (void) hipGetDevice(&dev);
    (void) hipGetDeviceProperties(&prop, dev);
    std::cout << "My PE: " << my_pe << " , Selected device: " << prop.name << std::endl;

    // Allocate memory on the ISHMEM symmetric heap on the device
    int *src = (int *) ishmem_malloc(N * sizeof(int));
    int *dst = (int *) ishmem_malloc(N * sizeof(int));

    // Initialize the src array on each device with the value pe
    hipLaunchKernelGGL(fill, dim3(1), dim3(64), 0, 0, src, my_pe);
    if (hipDeviceSynchronize() != hipSuccess) return EXIT_FAILURE;

    // Ensure completion of initialization
    ishmem_barrier_all();

    // Get data from the next device
    hipLaunchKernelGGL(get_from_next, dim3(1), dim3(64), 0, 0, dst, src, my_pe, npes);
    if (hipDeviceSynchronize() != hipSuccess) return EXIT_FAILURE;

    // Ensure completion of get operations and wait for other PEs
    ishmem_barrier_all();

    // Verify the data
    int *check = nullptr;
    if (hipHostMalloc((void **) &check, N * sizeof(int), 0) != hipSuccess) return EXIT_FAILURE;
    for (size_t i = 0; i < N; i++) check[i] = 1;
    hipLaunchKernelGGL(verify, dim3(1), dim3(64), 0, 0, dst, check, my_pe, npes);
    if (hipDeviceSynchronize() != hipSuccess) return EXIT_FAILURE;

    bool check_fail = false;
    for (size_t i = 0; i < N; i++)
        if (check[i]) {
            std::cerr << "PE: " << my_pe << " ISHMEM get failed at index: " << i << std::endl;
            check_fail = true;
        }

    if (!check_fail)
        std::cout << my_pe << " PE successfully received the data using ISHMEM get." << std::endl;
    std::cout << "PE#" << my_pe << (check_fail ? " FAILURE" : " SUCCESS") << " npes " << npes << std::endl;

    // Free the symmetric heap memory and check buffer
    ishmem_free(src);
    ishmem_free(dst);
    (void) hipHostFree(check);

    ishmem_finalize();

    return check_fail ? EXIT_FAILURE : EXIT_SUCCESS;
}
